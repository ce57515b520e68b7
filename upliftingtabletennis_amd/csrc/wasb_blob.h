// The WASB / HRNet weight blob (layout: include/ttup.h; order = upliftingtabletennis_amd.arch.hrnet_convs) parsed into folded convs:
// eval-mode BatchNorm goes into the weights and the bias here.  Host code without a HIP include, as csrc/wasb_graph.h; included by
// csrc/wasb_net.hip and by tests/helpers/host_wasb_graph.cpp.
#pragma once
#include "wasb_graph.h"
#include <math.h>
#include <string.h>

namespace ttup {

struct BlobReader {
    const char* p; size_t left;
    bool read(void* dst, size_t n) { if (n > left) return false; memcpy(dst, p, n); p += n; left -= n; return true; }
};

inline int parse_blob(const void* blob, size_t bytes, std::vector<FoldedConv>* out, int* in_ch, int* head_out,
                      std::vector<float>* head_w, std::vector<float>* head_b) {
    BlobReader r{(const char*)blob, bytes};
    char magic[8]; int hdr[4];
    TTUP_REQUIRE(r.read(magic, 8) && memcmp(magic, "TTUPWSB1", 8) == 0, TTUP_EFORMAT, "wasb blob: bad magic");
    TTUP_REQUIRE(r.read(hdr, sizeof hdr), TTUP_EFORMAT, "wasb blob: truncated header");
    const int n = hdr[0];
    *in_ch = hdr[1]; *head_out = hdr[2];
    TTUP_REQUIRE(n == WASB_CONVS, TTUP_EFORMAT, "wasb blob: expected %d convs, got %d", WASB_CONVS, n);
    for (int i = 0; i < n; ++i) {
        int h[8];
        TTUP_REQUIRE(r.read(h, sizeof h), TTUP_EFORMAT, "wasb blob: truncated at conv %d", i);
        FoldedConv c; c.cout = h[0]; c.cin = h[1]; c.k = h[2]; c.stride = h[3];
        const int has_bn = h[4], has_bias = h[5];
        TTUP_REQUIRE(c.cout > 0 && c.cout <= 128 && c.cin > 0 && c.cin <= 128 && (c.k == 1 || c.k == 3), TTUP_EFORMAT,
                     "wasb blob: conv %d has unsupported shape %dx%dx%d", i, c.cout, c.cin, c.k);
        const size_t nw = (size_t)c.cout * c.cin * c.k * c.k;
        c.w.resize(nw); c.bias.assign(c.cout, 0.f);
        TTUP_REQUIRE(r.read(c.w.data(), nw * 4), TTUP_EFORMAT, "wasb blob: truncated weights of conv %d", i);
        if (has_bias) TTUP_REQUIRE(r.read(c.bias.data(), c.cout * 4), TTUP_EFORMAT, "wasb blob: truncated bias of conv %d", i);
        if (has_bn) {
            std::vector<float> bn(4 * c.cout);
            TTUP_REQUIRE(r.read(bn.data(), bn.size() * 4), TTUP_EFORMAT, "wasb blob: truncated BN of conv %d", i);
            const float *gamma = bn.data(), *beta = gamma + c.cout, *mean = beta + c.cout, *var = mean + c.cout;
            const size_t per = (size_t)c.cin * c.k * c.k;
            for (int o = 0; o < c.cout; ++o) {
                // y = (conv(x)+b - mean) * gamma / sqrt(var + eps) + beta, eps = 1e-5 (nn.BatchNorm2d default)
                const double s = (double)gamma[o] / sqrt((double)var[o] + 1e-5);
                for (size_t j = 0; j < per; ++j) c.w[o * per + j] = (float)((double)c.w[o * per + j] * s);
                c.bias[o] = (float)(((double)c.bias[o] - (double)mean[o]) * s + (double)beta[o]);
            }
        }
        out->push_back(std::move(c));
    }
    TTUP_REQUIRE(r.left == 0, TTUP_EFORMAT, "wasb blob: %zu trailing bytes", r.left);
    const FoldedConv& head = out->back();
    TTUP_REQUIRE(head.k == 1 && head.cin == 16 && head.cout == *head_out, TTUP_EFORMAT, "wasb blob: unexpected head shape");
    *head_w = head.w; *head_b = head.bias;
    return TTUP_OK;
}

}  // namespace ttup
