// Host program over csrc/wasb_blob.h and csrc/wasb_graph.h for tests/test_wasb_graph_host.py
// (g++ -std=c++17 -O1 -g -fsanitize=address,undefined; run as a child process, never loaded into python).
//   parse BLOB              the parser's return code, its message, the header fields
//   fold BLOB I             conv I after the BatchNorm fold, as float bit patterns
//   plans BLOB H W [H W..]  the plan of every switch combination x {bf16, f32} at every size, as text
#include "../../upliftingtabletennis_amd/csrc/wasb_blob.h"
#include "../../upliftingtabletennis_amd/csrc/wasb_graph.h"
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static char g_error[512] = "";
namespace ttup {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}
}  // namespace ttup
using namespace ttup;

static uint64_t fnv(const std::vector<float>& v, uint64_t h) {
    const unsigned char* p = (const unsigned char*)v.data();
    for (size_t i = 0; i < v.size() * sizeof(float); ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}
static uint64_t weights_hash(const FoldedConv& f) { return fnv(f.bias, fnv(f.w, 14695981039346656037ull)); }

static void print_bits(const char* what, const std::vector<float>& v) {
    printf("%s", what);
    for (float x : v) { uint32_t u; memcpy(&u, &x, 4); printf(" %08x", u); }
    printf("\n");
}

static void print_plan(const GraphPlan& g, const std::vector<FoldedConv>& folded, const std::vector<uint64_t>& hash, int in_ch, int n_out, int H, int W, int dtype, int bits) {
    printf("plan dtype=%d in_ch=%d n_out=%d H=%d W=%d sw=%d%d%d%d%d%d rc=%d\n", dtype, in_ch, n_out, H, W, bits & 1, bits >> 1 & 1, bits >> 2 & 1,
           bits >> 3 & 1, bits >> 4 & 1, bits >> 5 & 1, g.rc);
    if (g.rc) { printf("error %s\nend\n", g_error); return; }
    printf("info consumed=%zu t_input=%d t_out=%d t_frames=%d fused_head=%d\n", g.consumed, g.t_input, g.t_out, g.t_frames, (int)g.fused_head);
    for (size_t i = 0; i < g.convs.size(); ++i) {
        const ConvRequest& r = g.convs[i];
        const FoldedConv& a = g.source_a(r, folded);
        printf("conv %zu a=%d b=%d synth=%d pad=%d cout=%d cin_total=%d c0=%d k=%d stride=%d a_shape=%d,%d,%d,%d ha=%016llx hb=%016llx\n", i, r.a, r.b, (int)r.synth,
               r.cin_pad, r.cout, r.cin_total, r.c0, r.k, r.stride, a.cout, a.cin, a.k, a.stride, (unsigned long long)(r.synth ? weights_hash(a) : hash[r.a]),
               (unsigned long long)(r.b >= 0 ? hash[r.b] : 0));
    }
    for (size_t i = 0; i < g.tensors.size(); ++i) printf("tensor %zu c=%d h=%d w=%d extra=%d\n", i, g.tensors[i].c, g.tensors[i].h, g.tensors[i].w, g.tensors[i].extra);
    for (size_t i = 0; i < g.ops.size(); ++i) {
        const Op& o = g.ops[i];
        printf("op %zu kind=%d n_chain=%d chain=%d,%d,%d,%d conv=%d conv2=%d conv3=%d conv1f=%d src0=%d src1=%d residual=%d dst=%d dst2=%d relu=%d "
               "n_terms=%d terms=%d,%d,%d shifts=%d,%d,%d res2=%d res3=%d sh3=%d head=%d lin16=%d lin16_dst=%d lin32=%d lin32_dst=%d pair=%d pair_dst=%d pair_relu=%d\n",
               i, (int)o.kind, o.n_chain, o.chain[0], o.chain[1], o.chain[2], o.chain[3], o.conv, o.conv2, o.conv3, o.conv1f, o.src0, o.src1, o.residual, o.dst, o.dst2,
               o.relu, o.n_terms, o.terms[0], o.terms[1], o.terms[2], o.shifts[0], o.shifts[1], o.shifts[2], o.res2, o.res3, o.sh3, o.head, o.lin16, o.lin16_dst,
               o.lin32, o.lin32_dst, o.pair, o.pair_dst, o.pair_relu);
    }
    for (const auto& t : g.taps) printf("tap %s %d\n", t.first.c_str(), t.second);
    printf("end\n");
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s parse|fold|plans BLOB ...\n", argv[0]); return 2; }
    std::vector<char> blob;
    {
        FILE* f = fopen(argv[2], "rb");
        if (!f) { perror(argv[2]); return 2; }
        char buf[1 << 16];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + n);
        fclose(f);
    }
    // the parser gets exactly the file's bytes in a heap block of exactly that size: a read past the end is an AddressSanitizer report
    char* exact = (char*)malloc(blob.size() ? blob.size() : 1);
    memcpy(exact, blob.data(), blob.size());
    std::vector<FoldedConv> folded;
    std::vector<float> head_w, head_b;
    int in_ch = 0, head_out = 0;
    const int rc = parse_blob(exact, blob.size(), &folded, &in_ch, &head_out, &head_w, &head_b);
    free(exact);
    const std::string cmd = argv[1];
    if (cmd == "parse" || rc != TTUP_OK) {
        printf("rc=%d\nerror=%s\nconvs=%zu in_ch=%d head_out=%d head_w=%zu head_b=%zu\n", rc, rc ? g_error : "", folded.size(), in_ch, head_out, head_w.size(), head_b.size());
        return 0;
    }
    if (cmd == "fold" && argc == 4) {
        const FoldedConv& f = folded.at(atoi(argv[3]));
        printf("shape %d %d %d %d\n", f.cout, f.cin, f.k, f.stride);
        print_bits("w", f.w);
        print_bits("bias", f.bias);
        return 0;
    }
    if (cmd == "plans" && argc >= 5 && argc % 2 == 1) {
        std::vector<uint64_t> hash;
        for (const FoldedConv& f : folded) hash.push_back(weights_hash(f));
        const int n_out = head_out == 3 ? 1 : head_out;          // as ttup_wasb_create: the ball detector returns the middle of its 3 channels
        for (int a = 3; a + 1 < argc; a += 2)
            for (int dtype : {TTUP_DTYPE_BF16, TTUP_DTYPE_F32})
                for (int bits = 0; bits < 64; ++bits) {
                    GraphSwitches sw;
                    sw.fuse = bits & 1; sw.fuse_sum = bits & 2; sw.fuse_lin = bits & 4; sw.pair = bits & 8; sw.stem = bits & 16; sw.frames_mode = bits & 32;
                    const int H = atoi(argv[a]), W = atoi(argv[a + 1]);
                    print_plan(build_graph(folded, in_ch, n_out, H, W, 8, dtype, sw), folded, hash, in_ch, n_out, H, W, dtype, bits);
                }
        return 0;
    }
    fprintf(stderr, "bad arguments\n");
    return 2;
}
