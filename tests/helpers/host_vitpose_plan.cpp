// Host program over csrc/vitpose_plan.h for tests/test_vitpose_plan_host.py
// (g++ -std=c++17 -O1 -g -fsanitize=address,undefined; run as a child process, never loaded into python).
//   layout IN_CH OUT_CH N_POS                    "tensors N total T", one "t offset count" line per tensor in blob order, then
//                                                "at NAME offset" for pos, blk5.qkvw, lnw, dc_w0, dc_b0, dc_w1, dc_b1, fin_w, fin_b
//   create BLOB H W MAX_BATCH MICRO IN_CH OUT_CH  check_create on the file's bytes: "rc N" and the message
//   create_resized BLOB DELTA H W ...            the same on the blob one byte short (DELTA -1) or long (+1)
//   buffers H W IN_CH OUT_CH [H W IN_CH OUT_CH ...]   the arena of every case x micro {1, 2, 8} x dtype {f32, bf16}: "cases N",
//                                                a "FAIL ..." line per violation, "failures N"
//   taps                                         "stages S depth D", then one "tap name first last cols bf16" line per tap
//   micro MAX_BATCH REQUESTED [...]              micro_batch of every pair, one per line
#include "../../upliftingtabletennis_amd/csrc/vitpose_plan.h"
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace ttup::vit;

static long long g_bad;
static char g_case[96];          // the case under check, for the FAIL lines
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s: ", g_case); printf(__VA_ARGS__); printf("\n"); ++g_bad; } } while (0)

static std::vector<char> read_file(const char* path) {
    std::vector<char> b;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    b.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (fread(b.data(), 1, b.size(), f) != b.size()) { fprintf(stderr, "short read of %s\n", path); exit(2); }
    fclose(f);
    return b;
}

static int create(std::vector<char> blob, int delta, char** a) {
    blob.resize(blob.size() + delta);          // a longer blob ends in a zero byte
    const Refusal r = check_create(blob.data(), blob.size(), atoi(a[0]), atoi(a[1]), atoi(a[2]), atoi(a[3]), atoi(a[4]), atoi(a[5]));
    printf("rc %d\n%s\n", r.rc, r.msg);
    return 0;
}

static void check_buffers(int h, int w, int in_ch, int out_ch, int micro, int dtype) {
    const size_t refine = 12345;          // any size: the plan takes the argmax workspace as it is given
    const BufferPlan p = plan_buffers(h, w, in_ch, out_ch, micro, dtype, refine);
    const size_t tokens = (size_t)micro * (h / 16) * (w / 16);
    snprintf(g_case, sizeof g_case, "h=%d w=%d in=%d out=%d micro=%d dtype=%d", h, w, in_ch, out_ch, micro, dtype);
    // 256-byte boundaries (2 MiB for a buffer that large), no overlap, inside the total
    std::vector<int> order;
    for (int b = 0; b < B_ARENA; ++b)
        if (p.bytes[b]) order.push_back(b);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return p.off[a] < p.off[b]; });
    for (size_t i = 0; i < order.size(); ++i) {
        const int b = order[i];
        const size_t end = i + 1 < order.size() ? p.off[order[i + 1]] : p.total;
        CHECK(p.off[b] % 256 == 0 && (p.bytes[b] < LARGE_ALIGN || p.off[b] % LARGE_ALIGN == 0), "buffer %d of %zu bytes at %zu", b, p.bytes[b], p.off[b]);
        CHECK(p.off[b] + p.bytes[b] <= end, "buffer %d at %zu + %zu runs past %zu", b, p.off[b], p.bytes[b], end);
    }
    // which buffers a handle has, and the ones whose size is stated outside the GEMM list
    for (int b : {B_X, B_STATS, B_QKV, B_ATT, B_HID, B_D2, B_HEAT, B_WS}) CHECK(p.bytes[b] > 0, "buffer %d is missing", b);
    CHECK((p.bytes[B_STATS64] > 0) == (dtype == 1), "stats64");
    CHECK(p.bytes[B_STATS64] == (dtype == 1 ? tokens * 2 * 8 : 0) && p.bytes[B_STATS] == tokens * 2 * 4, "statistics");
    CHECK(p.bytes[B_FRAMES] == (in_ch % 3 == 0 ? (size_t)(micro + in_ch / 3 - 1) * 3 * h * w * 4 : 0), "frames holds %zu bytes", p.bytes[B_FRAMES]);
    CHECK(p.bytes[B_HEAT] == tokens * 16 * out_ch * 4, "heat");
    CHECK(p.bytes[B_WS] >= refine, "argmax workspace");
    // every step of the list at batch = micro: its output fits, its dense input is there, it does not read what it writes
    for (int id = 0; id < G_COUNT; ++id) {
        const GemmSpec& g = GEMMS[id];
        const size_t K = g.K ? g.K : (size_t)in_ch * 256, M = g.m_per_token * tokens;
        const size_t out_size = g.bf16_out && dtype == 1 ? 2 : 4;
        CHECK(out_size == elem_size(g.out, dtype), "step %d writes %zu-byte elements into buffer %d", id, out_size, g.out);
        CHECK(g.out_per_token * tokens * g.N * out_size <= p.bytes[g.out], "step %d does not fit buffer %d", id, g.out);
        CHECK(g.am == A_DECONV ? g.out_per_token == 4 * g.m_per_token : g.out_per_token == g.m_per_token, "step %d rows", id);
        CHECK(g.in != g.out, "step %d reads the buffer it writes", id);
        if (g.in != B_IN) {
            const size_t row = g.am == A_DECONV ? K / 4 : K;          // a deconvolution phase gathers four pixels of K / 4 channels
            CHECK(M * row * elem_size(g.in, dtype) <= p.bytes[g.in], "step %d reads past buffer %d", id, g.in);
        }
        CHECK(((g.flags & E_RESID) != 0) == (g.out == B_X && id != G_PATCH), "step %d residual", id);
        CHECK(g.N % BN == 0 && K % BK == 0 && g.N % ttup::gemm16::TN == 0 && K % ttup::gemm16::TK == 0, "step %d: N %d K %zu off the tiles", id, g.N, K);
    }
}

int main(int argc, char** argv) {
    const char* cmd = argc > 1 ? argv[1] : "";
    if (!strcmp(cmd, "layout") && argc == 5) {
        const BlobLayout L = blob_layout(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
        printf("tensors %zu total %zu\n", L.t.size(), L.total);
        for (const BlobTensor& t : L.t) printf("t %zu %zu\n", t.offset, t.count);
        printf("at pos %zu\nat blk5.qkvw %zu\nat lnw %zu\nat dc_w0 %zu\nat dc_b0 %zu\nat dc_w1 %zu\nat dc_b1 %zu\nat fin_w %zu\nat fin_b %zu\n", L.pos, L.blk[5].qkvw, L.lnw,
               L.dc_w[0], L.dc_b[0], L.dc_w[1], L.dc_b[1], L.fin_w, L.fin_b);
        return 0;
    }
    if (!strcmp(cmd, "create") && argc == 9) return create(read_file(argv[2]), 0, argv + 3);
    if (!strcmp(cmd, "create_resized") && argc == 10) return create(read_file(argv[2]), atoi(argv[3]), argv + 4);
    if (!strcmp(cmd, "buffers") && argc >= 6 && argc % 4 == 2) {
        long long cases = 0;
        for (int i = 2; i < argc; i += 4)
            for (int micro : {1, 2, 8})
                for (int dtype : {0, 1}) { ++cases; check_buffers(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), micro, dtype); }
        printf("cases %lld\nfailures %lld\n", cases, g_bad);
        return 0;
    }
    if (!strcmp(cmd, "taps") && argc == 2) {
        printf("stages %d depth %d\n", STAGES, DEPTH);
        for (const Tap& t : TAPS) printf("tap %s %d %d %d %d\n", t.name, t.first, t.last, t.cols, (int)(elem_size(t.buf, 1) == 2));
        return 0;
    }
    if (!strcmp(cmd, "micro") && argc >= 4 && argc % 2 == 0) {
        for (int i = 2; i < argc; i += 2) printf("%d\n", micro_batch(atoi(argv[i]), atoi(argv[i + 1])));
        return 0;
    }
    fprintf(stderr, "usage: %s layout IN OUT N_POS | create BLOB H W MAXB MICRO IN OUT | create_resized BLOB DELTA H W MAXB MICRO IN OUT | buffers H W IN OUT ... | taps | micro MAXB REQ ...\n", argv[0]);
    return 2;
}
