// a6/a7: the 2D->3D uplift transformer (reference uplifting/model.py; the structure below is 'connectstage', mode 'dynamic',
// time_rotation 'new'; the other variants get_model builds are sequences of the same pieces, see forward_chunk) and the spin
// frame change (uplifting/helper.py:394-420), fp32 throughout.
//
// Structure (all tokens of a chunk of trajectories are processed as flat [tokens][D] arrays):
//   embed        BallEmbedding / TableEmbedding  model.py:105-158
//   table stage  (B*T) sequences x 14 tokens, 4 layers, RoPE on tokens 1..13 at fake times n/100 s  :360-384
//   time stage   B sequences x T tokens, depth-4 layers                                               :386-387
//   heads        MyHead 128->64->32->3                                                                :232-261
//   spin stage   cls token + T tokens, 4 layers, rotation head on the cls token                      :551-571
// This file is the forward's only translation unit and holds its host code: switches, blob loading, launch dispatch,
// forward_chunk, the hipGraph path, the C entry points.  The kernels are in headers private to it, one per family:
//   uplift_linear.h     linear_kernel (exact fp32 products on v_mfma_f32_16x16x4_f32), linear_x3_kernel (split bf16), small_linear_kernel
//   uplift_attention.h  attention_kernel (scalar, online softmax), attention_mfma_kernel / attention_mfma8_kernel (fp32 matrix pipe)
//   uplift_blocks.h     mlp_block_x3_kernel, mlp_block8_x3_kernel, qkv_block8_x3_kernel, attn_block_x3_kernel (fused layer halves)
//   uplift_stage.h      stage_x3_kernel (all layers of a stage of short sequences in one launch)
//   uplift_embed.h      strip_cls3_kernel, rope_index_kernel, stacked_embed_kernel, embed3_cls_kernel
#include "no_packed_fp32_begin.h"      // this unit's kernels run beside the CNN's chain kernels: no packed fp32 (common.h)
#include "common.h"
#include "uplift_net.h"
#include "uplift_x3.h"
#include "uplift_tokens.h"
#include <math.h>
#include <string.h>
#include <memory>
#include <vector>

using namespace ttup;
using namespace ttup::upl;

#include "uplift_linear.h"
#include "uplift_attention.h"
#include "uplift_blocks.h"
#include "uplift_stage.h"
#include "uplift_embed.h"

namespace {

// The environment switches (README, "knobs"), all read together, once per process, on the first use of any of them, through
// env_set() / env_ll() (common.h); TTUP_UPLIFT_NO_GRAPH is sampled through env_set() at every handle creation, TTUP_DEBUG where its
// message is printed.
struct Switches {
    bool f32_exact = env_set("TTUP_F32_EXACT");                          // fp32-MFMA kernels throughout, scalar attention
    bool unfused = env_set("TTUP_UPLIFT_UNFUSED");                       // one launch per linear layer
    bool scalar_attention = env_set("TTUP_UPLIFT_SCALAR_ATTENTION");
    bool attention_2pass = env_set("TTUP_UPLIFT_ATTENTION_2PASS");       // the first matrix-pipe form (cross-check)
    bool qkv_linear = env_set("TTUP_UPLIFT_QKV_LINEAR");                 // the general linear kernel instead of qkv_block8_x3_kernel (cross-check)
    bool mlp_4waves = env_set("TTUP_UPLIFT_MLP_4WAVES");                 // mlp_block_x3_kernel: 4 waves, two n-tiles each
    bool no_stage = env_set("TTUP_UPLIFT_NO_STAGE");
    bool assemble = env_set("TTUP_UPLIFT_ASSEMBLE");                     // build the table stage's token tensor in memory
    bool stacked_per_token = env_set("TTUP_UPLIFT_STACKED_PER_TOKEN");   // the other summation order (cross-check)
    bool stage_stamps = env_set("TTUP_STAGE_STAMPS");
    long long stage_wg = env_ll("TTUP_UPLIFT_STAGE_WG", 1ll << 40);         // largest launch (workgroups) stage_x3_kernel is used for
};
const Switches& switches() { static const Switches s; return s; }

struct Reader {
    const char* p; size_t left;
    std::vector<float>* keep = nullptr;          // when set, every record is also appended here (the plain fp32 copy, uplift_net.h)
    bool take(std::vector<float>* v, size_t expect) {
        int n;
        if (left < 4) return false;
        memcpy(&n, p, 4); p += 4; left -= 4;
        if ((size_t)n != expect || left < expect * 4) return false;
        v->resize(expect); memcpy(v->data(), p, expect * 4); p += expect * 4; left -= expect * 4;
        if (keep) keep->insert(keep->end(), v->begin(), v->end());
        return true;
    }
};

// (every fp32 buffer carries 16 bytes of padding, the bf16 weight image none)
template <typename T>
int dev_copy(ttup_uplift* net, const std::vector<T>& v, T** out, size_t pad_bytes = 16) {
    void* d = nullptr;
    TTUP_HIP_CHECK(hipMalloc(&d, v.size() * sizeof(T) + pad_bytes));
    net->allocs.push_back(d);
    TTUP_HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (T*)d;
    return TTUP_OK;
}
// uninitialised device buffers of `floats` fp32 words (+ the padding) each, allocated in the order given; an entry of 0 words is skipped
struct Buf { void** p; size_t floats; };
int dev_alloc(ttup_uplift* net, std::initializer_list<Buf> bufs) {
    for (const Buf& b : bufs) {
        if (b.floats == 0) continue;
        TTUP_HIP_CHECK(hipMalloc(b.p, b.floats * 4 + 16));
        net->allocs.push_back(*b.p);
    }
    return TTUP_OK;
}

// W [n][k] as the A fragments of v_mfma_f32_16x16x4_f32, [ntile][k/16][64 lanes][4] in linear_kernel's K permutation; rows past n are 0
std::vector<float> pack_f32_fragments(const std::vector<float>& w, int n, int k) {
    const int ntiles = (n + 15) / 16, ks4 = k / 16, kq = k / 4;
    std::vector<float> p((size_t)ntiles * ks4 * 64 * 4, 0.f);
    for (int nt = 0; nt < ntiles; ++nt)
        for (int s4 = 0; s4 < ks4; ++s4)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 4; ++j) {
                    const int row = nt * 16 + (l & 15), kk = (l >> 4) * kq + s4 * 4 + j;
                    p[(((size_t)nt * ks4 + s4) * 64 + l) * 4 + j] = row < n ? w[(size_t)row * k + kk] : 0.f;
                }
    return p;
}
// W [n][k] split exactly into three bf16 parts, as the A fragments of v_mfma_f32_16x16x32_bf16: [ntile][k/32][plane][64 lanes][8]
std::vector<uint16_t> pack_split_bf16(const std::vector<float>& w, int n, int k) {
    const int ntiles = (n + 15) / 16, ks = k / 32;
    std::vector<uint16_t> p3((size_t)ntiles * ks * 3 * 64 * 8, 0);
    for (int nt = 0; nt < ntiles; ++nt)
        for (int s_ = 0; s_ < ks; ++s_)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int row = nt * 16 + (l & 15), kk = s_ * 32 + (l >> 4) * 8 + j;
                    const float v = row < n ? w[(size_t)row * k + kk] : 0.f;
                    const bf16_t a0 = f32_to_bf16(v);
                    const float r1 = v - bf16_to_f32(a0);
                    const bf16_t a1 = f32_to_bf16(r1);
                    const bf16_t a2 = f32_to_bf16(r1 - bf16_to_f32(a1));
                    const size_t base = (((size_t)nt * ks + s_) * 3) * 512 + (size_t)l * 8 + j;
                    p3[base] = a0; p3[base + 512] = a1; p3[base + 1024] = a2;
                }
    return p3;
}

int make_linear(ttup_uplift* net, Reader& r, int n, int k, bool has_bias, Linear* L) {
    std::vector<float> w, b;
    TTUP_REQUIRE(r.take(&w, (size_t)n * k), TTUP_EFORMAT, "uplift blob: bad weight record (%dx%d)", n, k);
    if (has_bias) TTUP_REQUIRE(r.take(&b, n), TTUP_EFORMAT, "uplift blob: bad bias record (%d)", n);
    L->n = n; L->k = k; L->mfma = (k % 16 == 0);
    int rc;
    if (L->mfma) {
        if ((rc = dev_copy(net, pack_f32_fragments(w, n, k), &L->w_dev))) return rc;
        if (k == 128 && n % 4 == 0 && (rc = dev_copy(net, pack_split_bf16(w, n, k), &L->w3_dev, 0))) return rc;
    } else if ((rc = dev_copy(net, w, &L->w_dev))) return rc;
    return has_bias ? dev_copy(net, b, &L->b_dev) : TTUP_OK;
}

// a [n][k] weight record stored transposed [k][n] (+ its bias) for the per-column kernels (stacked_embed_kernel, embed3_cls_kernel)
int make_linear_t(ttup_uplift* net, Reader& r, int n, int k, float** wt, float** b) {
    std::vector<float> w, bias;
    TTUP_REQUIRE(r.take(&w, (size_t)n * k), TTUP_EFORMAT, "uplift blob: bad weight record (%dx%d)", n, k);
    TTUP_REQUIRE(r.take(&bias, n), TTUP_EFORMAT, "uplift blob: bad bias record (%d)", n);
    std::vector<float> t((size_t)n * k);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < k; ++j) t[(size_t)j * n + i] = w[(size_t)i * k + j];
    if (int rc = dev_copy(net, t, wt)) return rc;
    return dev_copy(net, bias, b);
}

int make_vec(ttup_uplift* net, Reader& r, int n, float** out) {
    std::vector<float> v;
    TTUP_REQUIRE(r.take(&v, n), TTUP_EFORMAT, "uplift blob: bad vector record (%d)", n);
    return dev_copy(net, v, out);
}

int make_layer(ttup_uplift* net, Reader& r, Layer* L) {
    const int D = net->D;
    int rc;
    if ((rc = make_linear(net, r, 3 * D, D, true, &L->qkv))) return rc;
    if ((rc = make_linear(net, r, D, D, false, &L->proj))) return rc;      // no bias: model.py:268 / :162
    if ((rc = make_linear(net, r, D, D, true, &L->fc1))) return rc;
    if ((rc = make_linear(net, r, D, D, true, &L->fc2))) return rc;
    for (float** v : {&L->g1, &L->b1, &L->g2, &L->b2})
        if ((rc = make_vec(net, r, D, v))) return rc;
    return TTUP_OK;
}
int make_mlp2(ttup_uplift* net, Reader& r, int din, Mlp2* m) {
    if (int rc = make_linear(net, r, net->D, din, true, &m->fc1)) return rc;
    return make_linear(net, r, net->D, net->D, true, &m->fc2);
}
int make_head(ttup_uplift* net, Reader& r, Head* h) {
    const int D = net->D;
    if (int rc = make_linear(net, r, D / 2, D, true, &h->fc1)) return rc;
    if (int rc = make_linear(net, r, D / 4, D / 2, true, &h->fc2)) return rc;
    return make_linear(net, r, 3, D / 4, true, &h->fc3);
}

// a launch of a kernel that may ask for more than 64 KB of dynamic LDS: raise its limit (once per kernel and device), launch, check
template <typename... P, typename... A>
int launch_lds(void (*kernel)(P...), dim3 grid, dim3 block, size_t smem, hipStream_t st, A... args) {
    if (int rc = ensure_max_lds((const void*)kernel, 160 * 1024)) return rc;
    hipLaunchKernelGGL(kernel, grid, block, smem, st, args...);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

// linear_x3_kernel (X3) or linear_kernel <LN, NTW, MH> for the run-time choice of (LayerNorm, n-tiles per wave, 128-row tile)
template <bool X3, bool LN, int NTW, int MH>
int launch_linear_as(dim3 grid, size_t smem, hipStream_t st, const LinArgs& a, const uint16_t* w3) {
    if constexpr (X3) return launch_lds(linear_x3_kernel<LN, NTW, MH>, grid, dim3(256 * MH), smem, st, a, w3);
    else return launch_lds(linear_kernel<LN, NTW, MH>, grid, dim3(256 * MH), smem, st, a);
}
template <bool X3, bool LN, int MH>
int launch_linear_n(int ntw, dim3 grid, size_t smem, hipStream_t st, const LinArgs& a, const uint16_t* w3) {
    return ntw == 3 ? launch_linear_as<X3, LN, 3, MH>(grid, smem, st, a, w3) : ntw == 2 ? launch_linear_as<X3, LN, 2, MH>(grid, smem, st, a, w3)
                                                                                      : launch_linear_as<X3, LN, 1, MH>(grid, smem, st, a, w3);
}
template <bool X3>
int launch_linear(bool ln, bool big, int ntw, dim3 grid, size_t smem, hipStream_t st, const LinArgs& a, const uint16_t* w3) {
    if (ln) return big ? launch_linear_n<X3, true, 2>(ntw, grid, smem, st, a, w3) : launch_linear_n<X3, true, 1>(ntw, grid, smem, st, a, w3);
    return big ? launch_linear_n<X3, false, 2>(ntw, grid, smem, st, a, w3) : launch_linear_n<X3, false, 1>(ntw, grid, smem, st, a, w3);
}

int run_linear(const Linear& L, const float* x, int ldx, long long M, const float* gamma, const float* beta, int relu,
               const float* res, int ldr, float* out, int ldo, hipStream_t st) {
    if (M == 0) return TTUP_OK;
    if (!L.mfma) {
        TTUP_REQUIRE(!gamma && !res, TTUP_EINVAL, "small linear: LN/residual unsupported");
        return launch_1d(small_linear_kernel, M * L.n, st, x, ldx, L.w_dev, L.b_dev, out, ldo, M, L.n, L.k, relu);
    }
    LinArgs a;
    a.x = x; a.ldx = ldx; a.w = L.w_dev; a.bias = L.b_dev; a.gamma = gamma; a.beta = beta; a.res = res; a.ldr = ldr;
    a.out = out; a.ldo = ldo; a.M = (int)M; a.N = L.n; a.K = L.k; a.relu = relu;
    TTUP_REQUIRE(ldx % 4 == 0 && L.k <= 256, TTUP_EINVAL, "linear: row stride %d / K %d unsupported", ldx, L.k);
    // 128-row tiles once there are enough rows to fill the chip twice over, 64-row tiles below that
    const bool big = M >= 128 * 512;
    const int ntw = L.n > 128 ? 3 : L.n > 64 ? 2 : 1;
    const int bm = big ? 128 : 64;
    const dim3 grid((unsigned)((M + bm - 1) / bm), (unsigned)((L.n + 64 * ntw - 1) / (64 * ntw)));
    const bool x3 = L.w3_dev && !switches().f32_exact && ldo % 4 == 0 && (!res || ldr % 4 == 0);
    const size_t smem = x3 ? (size_t)3 * bm * 128 * sizeof(uint16_t) : (size_t)4 * bm * (L.k / 4 + 4) * sizeof(float);
    return x3 ? launch_linear<true>(gamma != nullptr, big, ntw, grid, smem, st, a, L.w3_dev)
              : launch_linear<false>(gamma != nullptr, big, ntw, grid, smem, st, a, nullptr);
}

template <int HD>
void launch_attention(const AttnArgs& a, hipStream_t st) {
    const int S = a.sv.S;
    const int P = S <= 16 ? 16 : S <= 32 ? 32 : S <= 64 ? 64 : 128;
    const int threads = P == 128 ? 128 : 64, G = threads / P;
    const size_t smem = ((size_t)G * (2 * S * HD + 16) + (size_t)G * S) * sizeof(float);
    const dim3 grid((unsigned)((a.n_seq + G - 1) / G), a.heads);
    switch (P) {
        case 16: hipLaunchKernelGGL((attention_kernel<HD, 16>), grid, dim3(threads), smem, st, a); break;
        case 32: hipLaunchKernelGGL((attention_kernel<HD, 32>), grid, dim3(threads), smem, st, a); break;
        case 64: hipLaunchKernelGGL((attention_kernel<HD, 64>), grid, dim3(threads), smem, st, a); break;
        default: hipLaunchKernelGGL((attention_kernel<HD, 128>), grid, dim3(threads), smem, st, a); break;
    }
}

// The longest sequence run_attention serves for this handle: 512 tokens (32 key tiles, 148 KB of LDS) on the matrix-pipe kernels, which
// take D = 128 / head_dim 32 unless a switch selects the scalar kernel; else what fits attention_kernel's 64 KB of LDS with one sequence
// per workgroup, (2 S hd + 16 + S) floats: 962 / 496 / 334 / 251 tokens for head dims 8 / 16 / 24 / 32.
constexpr int ATTN_MFMA_MAX_S = 512;
int max_attention_seq(const ttup_uplift* net) {
    const Switches& sw = switches();
    if (net->hd == 32 && net->D == 128 && !sw.scalar_attention && !sw.f32_exact) return ATTN_MFMA_MAX_S;
    return (64 * 1024 / (int)sizeof(float) - 16) / (2 * net->hd + 1);
}

int run_attention(ttup_uplift* net, const float* qkv, float* out, int n_seq, const SeqView& sv, hipStream_t st) {
    const int S = sv.S;
    const AttnArgs a{qkv, out, n_seq, net->D, net->heads, net->hd, sv};
    const Switches& sw = switches();
    const bool scalar_attn = sw.scalar_attention || sw.f32_exact;
    if (net->hd == 32 && net->D == 128 && S > 16 && S <= ATTN_MFMA_MAX_S && !scalar_attn) {
        const AttnMArgs m{qkv, out, sv, n_seq};
        const int KT = (S + 15) / 16;
        if (KT <= 8 && !sw.attention_2pass) {
            const size_t smem8 = ((size_t)KT * 16 * ATTM_KS + (size_t)32 * (KT * 16 + 4) + 64) * sizeof(float);
            if (KT <= 4) hipLaunchKernelGGL(attention_mfma8_kernel<1>, dim3((KT + 3) / 4, net->heads, n_seq), dim3(256), smem8, st, m);
            else hipLaunchKernelGGL(attention_mfma8_kernel<2>, dim3((KT + 3) / 4, net->heads, n_seq), dim3(256), smem8, st, m);
            TTUP_LAUNCH_CHECK();
            return TTUP_OK;
        }
        const size_t smem = ((size_t)2 * KT * 16 * ATTM_KS + 64) * sizeof(float);
        return launch_lds(attention_mfma_kernel, dim3((KT + 3) / 4, net->heads, n_seq), dim3(256), smem, st, m);
    }
    TTUP_REQUIRE(((size_t)2 * S * net->hd + 16 + S) * sizeof(float) <= 64 * 1024, TTUP_EINVAL, "attention: sequence length %d too long", S);
    switch (net->hd) {
        case 8: launch_attention<8>(a, st); break;
        case 16: launch_attention<16>(a, st); break;
        case 24: launch_attention<24>(a, st); break;
        case 32: launch_attention<32>(a, st); break;
        default: set_error("attention: head_dim %d unsupported", net->hd); return TTUP_EINVAL;
    }
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

// SimpleStaticLayer.forward (model.py:278-300) on x [n_seq*S][D] in place (x2 is scratch of the same size)
int run_layer(ttup_uplift* net, const Layer& L, float* x, long long tokens, int n_seq, const SeqView& sv, hipStream_t st) {
    const int D = net->D, S = sv.S;
    int rc;
    const Switches& sw = switches();
    const bool fused = !sw.f32_exact && !sw.unfused;
    if (D == 128 && net->heads == 4 && S <= 16 && L.qkv.w3_dev && fused) {
        // short sequences (table stage): LN + qkv + RoPE + attention in one kernel, qkv never leaves the CU (attn_block_x3_kernel)
        AttnBlockArgs a;
        a.x = x; a.att = net->att; a.n_seq = n_seq; a.w_qkv = L.qkv.w3_dev; a.b_qkv = L.qkv.b_dev; a.g1 = L.g1; a.b1 = L.b1;
        a.sv = sv;
        const int seqs = 64 / S;
        const size_t smem = (size_t)64 * ATTN_QS * sizeof(float);          // (>= the 48 KB of the three split planes it first holds)
        const dim3 grid((unsigned)((n_seq + seqs - 1) / seqs));
        if ((rc = launch_lds(attn_block_x3_kernel, grid, dim3(512), smem, st, a))) return rc;
    } else {
        // (small launches only: on a full device the general kernel -- 128-token tiles, two workgroups per 128 x 384 block -- is 4 % ahead,
        // B = 10 000: 65.2 k vs 62.8 k trajectories/s; three 121-token trajectories: 0.712 -> 0.689 ms with this one)
        if (D == 128 && L.qkv.w3_dev && L.qkv.n == 384 && fused && !sw.qkv_linear && tokens <= 64 * 256) {
            QkvArgs qa{x, net->qkv, tokens, L.qkv.w3_dev, L.qkv.b_dev, L.g1, L.b1};
            hipLaunchKernelGGL(qkv_block8_x3_kernel, dim3((unsigned)((tokens + 63) / 64)), dim3(512), (size_t)3 * 64 * 128 * sizeof(uint16_t), st, qa);
            TTUP_LAUNCH_CHECK();
        } else if ((rc = run_linear(L.qkv, x, D, tokens, L.g1, L.b1, 0, nullptr, 0, net->qkv, 3 * D, st))) return rc;
        if ((rc = run_attention(net, net->qkv, net->att, n_seq, sv, st))) return rc;
    }
    if (D == 128 && L.proj.w3_dev && L.fc1.w3_dev && L.fc2.w3_dev && fused) {
        // x = fc2(relu(fc1(LN(proj(att) + x)))) + (proj(att) + x) in one pass over the tokens (mlp_block_x3_kernel)
        MlpArgs a;
        a.att = net->att; a.x = x; a.M = tokens;
        a.w_proj = L.proj.w3_dev; a.w_fc1 = L.fc1.w3_dev; a.w_fc2 = L.fc2.w3_dev;
        a.g2 = L.g2; a.b2 = L.b2; a.bias1 = L.fc1.b_dev; a.bias2 = L.fc2.b_dev;
        // 64-token tiles (80 KB of LDS: two workgroups per CU) also for large token counts: 2 % faster at B = 10 000 than the 128-token
        // tile (160 KB, one workgroup per CU) although every tile then streams the weights again
        constexpr int bm = 64;
        const size_t smem = (size_t)3 * bm * 128 * sizeof(uint16_t) + (size_t)bm * 128 * sizeof(float);
        const dim3 grid((unsigned)((tokens + bm - 1) / bm));
        if (sw.mlp_4waves) return launch_lds(mlp_block_x3_kernel, grid, dim3(256), smem, st, a);
        return launch_lds(mlp_block8_x3_kernel, grid, dim3(512), smem, st, a);
    }
    if ((rc = run_linear(L.proj, net->att, D, tokens, nullptr, nullptr, 0, x, D, net->x2, D, st))) return rc;       // x2 = proj(att) + x
    if ((rc = run_linear(L.fc1, net->x2, D, tokens, L.g2, L.b2, 1, nullptr, 0, net->hid, D, st))) return rc;          // hid = relu(fc1(LN(x2)))
    return run_linear(L.fc2, net->hid, D, tokens, nullptr, nullptr, 0, net->x2, D, x, D, st);                       // x = fc2(hid) + x2
}

// the layers' weight pointers for stage_x3_kernel (left empty when a layer has no split-bf16 image or the table would not fit)
void make_stage(ttup_uplift* net, const std::vector<Layer>& layers, std::vector<StageLayerW>* out) {
    out->clear();
    if (layers.empty() || layers.size() > (size_t)STAGE_MAX_LAYERS || net->D != 128 || net->heads != 4) return;
    for (const Layer& L : layers) {
        if (!L.qkv.w3_dev || !L.proj.w3_dev || !L.fc1.w3_dev || !L.fc2.w3_dev) { out->clear(); return; }
        out->push_back(StageLayerW{L.qkv.w3_dev, L.proj.w3_dev, L.fc1.w3_dev, L.fc2.w3_dev, L.qkv.b_dev, L.g1, L.b1, L.g2, L.b2, L.fc1.b_dev, L.fc2.b_dev});
    }
}

// TTUP_STAGE_STAMPS, a debugging aid (synchronises; skipped while the stream is being captured): cycles between the phase boundaries of
// the LAST layer, wave 0 of workgroup 0
int print_stage_stamps(const StageArgs& a, long long wgs, hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cs);
    if (cs != hipStreamCaptureStatusNone) return TTUP_OK;
    std::vector<long long> h((size_t)a.n_layers * 12);
    TTUP_HIP_CHECK(hipStreamSynchronize(st));
    TTUP_HIP_CHECK(hipMemcpy(h.data(), a.stamps, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    const long long* t = h.data() + (size_t)(a.n_layers - 1) * 12;
    fprintf(stderr, "stage S=%d n_seq=%d wgs=%lld layers=%d: whole stage %lld clk; last layer: ln1 %lld qkv %lld wait %lld attn %lld wait %lld att->planes %lld proj %lld ln2 %lld fc1+split %lld fc2 %lld wait %lld\n",
            a.sv.S, (int)a.n_seq, wgs, a.n_layers, t[11] - h[0], t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4], t[6] - t[5],
            t[7] - t[6], t[8] - t[7], t[9] - t[8], t[10] - t[9], t[11] - t[10]);
    return TTUP_OK;
}

// Every layer of a stage: one stage_x3_kernel launch when the sequences fit a 64-token tile (the table stage always; the temporal
// and spin stages of clips of up to 63 frames), else layer by layer.  The kernel holds 156 KB of LDS -- one workgroup per CU -- and
// still beats the per-layer kernels (two per CU) on a full device: 55 k cycles per 64-token layer against 19 k (attention block,
// bound by the L1 traffic of its weight fragments: every m-tile wave streams its head's weights) + 38 k (MLP block); B = 10 000,
// T = 120: 50.1 k -> 55.4 k trajectories/s, B = 4096, T = 50: 123 k -> 149 k.  TTUP_UPLIFT_STAGE_WG caps the launch size it is used for.
int run_stage(ttup_uplift* net, const std::vector<Layer>& layers, const std::vector<StageLayerW>& stage, float* x, long long tokens, int n_seq, const SeqView& sv,
              hipStream_t st, const float* table_tok = nullptr, int T = 0, int NT = 0, bool* fused_tokens = nullptr) {
    // (table_tok: the table stage.  When the stage kernel runs, `x` is then the ball-token tensor [n_seq][D], read and written in
    // place, and *fused_tokens = true; otherwise the caller assembles / gathers around the per-layer kernels, which get `x` as usual)
    if (fused_tokens) *fused_tokens = false;
    const int S = sv.S;
    const Switches& sw = switches();
    const bool off = sw.f32_exact || sw.unfused || sw.no_stage;
    if (!stage.empty() && !off && S <= 64 && n_seq > 0 && (64 / S) * ((S + 3) & ~3) <= STAGE_VS) {          // (V^T holds every sequence of the tile at a multiple of 4)
        const int seqs = 64 / S;
        const long long wgs = ((long long)n_seq + seqs - 1) / seqs;
        if (wgs <= sw.stage_wg) {
            StageArgs a;
            a.x = x; a.n_seq = n_seq; a.n_layers = (int)layers.size();
            memcpy(a.layers, stage.data(), stage.size() * sizeof(StageLayerW));
            a.sv = sv;
            a.table_tok = table_tok; a.T = T; a.NT = NT;
            if (fused_tokens) *fused_tokens = table_tok != nullptr;
            int rc;
            if (sw.stage_stamps && !net->stage_stamps &&
                (rc = dev_alloc(net, {{(void**)&net->stage_stamps, STAGE_MAX_LAYERS * 12 * sizeof(long long) / 4}}))) return rc;
            a.stamps = sw.stage_stamps ? net->stage_stamps : nullptr;
            if ((rc = launch_lds(stage_x3_kernel, dim3((unsigned)wgs), dim3(512), STAGE_LDS, st, a))) return rc;
            if (sw.stage_stamps && (rc = print_stage_stamps(a, wgs, st))) return rc;
            net->stage_launches++;
            return TTUP_OK;
        }
    }
    if (table_tok) return TTUP_OK;          // declined (*fused_tokens is false, nothing launched): the caller assembles the tokens and calls again
    for (const Layer& L : layers)
        if (int rc = run_layer(net, L, x, tokens, n_seq, sv, st)) return rc;
    return TTUP_OK;
}

int run_head(ttup_uplift* net, const Head& h, const float* x, int ldx, long long M, float* out, hipStream_t st) {
    const int D = net->D;
    if (int rc = run_linear(h.fc1, x, ldx, M, nullptr, nullptr, 1, nullptr, 0, net->hid, D / 2, st)) return rc;
    if (int rc = run_linear(h.fc2, net->hid, D / 2, M, nullptr, nullptr, 1, nullptr, 0, net->att, D / 4, st)) return rc;
    return run_linear(h.fc3, net->att, D / 4, M, nullptr, nullptr, 0, nullptr, 0, out, 3, st);
}

// One chunk of trajectories.  Every variant is a sequence of the same pieces (model.py:303-571):
//   tokens    dynamic: ball_embed (2 -> D -> D), table_embed, table stage;  stacked / originalmethod: stacked_embed_kernel + fc2;
//             free: ball_embed alone
//   connectstage  temporal stage (depth-4 layers) -> position head;  cls + tokens   -> spin stage (4 layers) -> rotation head
//   multistage    temporal stage (depth-4 layers) -> position head;  cls + embed(pos) (embed3_cls_kernel) -> spin stage -> rotation head
//   singlestage   cls + tokens -> one stage of all `depth` layers -> rotation head on row 0, position head on rows 1..T
// time_rotation 'old' reads the fixed by-index (cos, sin) table (row stride 0 between sequences) instead of the per-forward one.
int forward_chunk(ttup_uplift* net, const float* ball, const float* table, const float* mask, const float* times, int B, int T,
                  float* rot, float* pos, hipStream_t st) {
    const int D = net->D, NT = net->n_table, S1 = NT + 1;
    int rc;
    if ((rc = launch_1d(prepare_kernel<true>, (long long)B * T + (long long)B * NT, st, mask, table, net->m1, net->m2, net->tmask, net->txy, B, T, NT, net->flags_dev))) return rc;
    const float2* rope = net->rope_index;
    const int rope_stride = net->rot_old ? 0 : T;
    if (!net->rot_old) {
        const long long n = (long long)B * T * (net->hd / 2);
        if ((rc = launch_1d(rope_table_kernel, n, st, times, net->inv_freq_dev, net->rope, net->hd / 2, n))) return rc;
        rope = net->rope;
    }
    // the sequences of the three stages: (b, t) -> [ball token, 13 table tokens] at fake times; b -> T tokens; b -> cls + T tokens
    const float scale = 1.0f / sqrtf((float)net->hd);
    const SeqView sv_table{net->tmask, net->table_rope, S1, 1, T, 1, 0, scale};
    const SeqView sv_time{net->m1, rope, T, 0, 1, 1, rope_stride, scale}, sv_cls{net->m2, rope, T + 1, 1, 1, 1, rope_stride, scale};
    // embeddings
    if (net->mode == MODE_STACKED || net->mode == MODE_ORIGINAL) {
        const dim3 grid((unsigned)B, (unsigned)((T + STACKED_TOKENS - 1) / STACKED_TOKENS));
        const int tw = net->mode == MODE_STACKED ? 3 : 2;
        if (switches().stacked_per_token) hipLaunchKernelGGL(stacked_embed_kernel<true>, grid, dim3(256), 0, st, ball, table, net->stacked_wt, net->stacked_b, net->h1, T, D, tw);
        else hipLaunchKernelGGL(stacked_embed_kernel<false>, grid, dim3(256), 0, st, ball, table, net->stacked_wt, net->stacked_b, net->h1, T, D, tw);
        TTUP_LAUNCH_CHECK();
    } else if ((rc = run_linear(net->ball_embed.fc1, ball, 2, (long long)B * T, nullptr, nullptr, 1, nullptr, 0, net->h1, D, st))) return rc;
    if ((rc = run_linear(net->ball_embed.fc2, net->h1, D, (long long)B * T, nullptr, nullptr, 0, nullptr, 0, net->tok, D, st))) return rc;
    if (net->mode == MODE_DYNAMIC) {
        if ((rc = run_linear(net->table_embed.fc1, net->txy, 2, (long long)B * NT, nullptr, nullptr, 1, nullptr, 0, net->h1, D, st))) return rc;
        if ((rc = run_linear(net->table_embed.fc2, net->h1, D, (long long)B * NT, nullptr, nullptr, 0, nullptr, 0, net->ttok, D, st))) return rc;
        // table stage: every (b, t) is a 14-token sequence [ball token, 13 table tokens]; its row 0 replaces the ball token afterwards
        const long long tok1 = (long long)B * T * S1;
        bool fused = false;
        // stage kernel: reads the two token tensors itself and writes row 0 only (nothing has been launched if it declines)
        if (!switches().assemble && (rc = run_stage(net, net->pos_layers, net->stage_pos, net->tok, tok1, B * T, sv_table, st, net->ttok, T, NT, &fused))) return rc;
        if (!fused) {
            const long long total = tok1 * D;
            if ((rc = launch_1d(assemble_table_kernel, total, st, net->tok, net->ttok, net->x, T, NT, D, total))) return rc;
            if ((rc = run_stage(net, net->pos_layers, net->stage_pos, net->x, tok1, B * T, sv_table, st))) return rc;
            const long long total2 = (long long)B * T * D;
            if ((rc = launch_1d(gather_rows_kernel, total2, st, net->x, net->tok, D, S1, total2))) return rc;
        }
    }
    if (net->name != NAME_SINGLE) {
        // temporal stage (tok is [B*T][D])
        if ((rc = run_stage(net, net->layers, net->stage_first, net->tok, (long long)B * T, B, sv_time, st))) return rc;
        if ((rc = run_head(net, net->position_head, net->tok, D, (long long)B * T, pos, st))) return rc;
    }
    // cls token in front of every sequence (x is [B*(T+1)][D])
    if (net->name == NAME_MULTI) {
        const long long tokens = (long long)B * T;
        hipLaunchKernelGGL(embed3_cls_kernel, dim3((unsigned)((tokens + EMBED3_TOKENS - 1) / EMBED3_TOKENS)), dim3(256), 0, st,
                           pos, net->embed_w1t, net->embed_b1, net->embed_w2t, net->embed_b2, net->cls_dev, net->x, T, D, tokens);
        TTUP_LAUNCH_CHECK();
    } else {
        const long long total = (long long)B * (T + 1) * D;
        if ((rc = launch_1d(prepend_cls_kernel, total, st, net->tok, net->cls_dev, net->x, T, D, total))) return rc;
    }
    if (net->name == NAME_SINGLE) {
        if ((rc = run_stage(net, net->layers, net->stage_first, net->x, (long long)B * (T + 1), B, sv_cls, st))) return rc;
        // position head on every row, the cls rows dropped afterwards (3 floats a row; the head's rows must be evenly spaced)
        if ((rc = run_head(net, net->position_head, net->x, D, (long long)B * (T + 1), net->pos_rows, st))) return rc;
        const long long total = (long long)B * T * 3;
        if ((rc = launch_1d(strip_cls3_kernel, total, st, net->pos_rows, pos, T, total))) return rc;
    } else if ((rc = run_stage(net, net->second, net->stage_second, net->x, (long long)B * (T + 1), B, sv_cls, st))) return rc;
    // rotation head on the cls rows (row stride (T+1)*D)
    return run_head(net, net->rotation_head, net->x, (T + 1) * D, B, rot, st);
}

// ---- ttup_uplift_create in four steps: header, weight records, scratch, graph buffers
int parse_header(const void* blob, int max_batch, int max_len, ttup_uplift* net) {
    int hdr[8];
    memcpy(hdr, (const char*)blob + 8, sizeof hdr);
    net->D = hdr[0]; net->heads = hdr[1]; net->n_table = hdr[5];
    const int n_pos = hdr[2], n_first = hdr[3], n_second = hdr[4];
    net->name = hdr[6] & 15; net->mode = hdr[6] >> 4; net->rot_old = hdr[7] == 1;
    TTUP_REQUIRE(hdr[6] >= 0 && net->name <= NAME_SINGLE && net->mode <= MODE_FREE && (hdr[7] == 0 || hdr[7] == 1) &&
                 (net->mode == MODE_FREE ? net->name == NAME_SINGLE : net->mode != MODE_ORIGINAL || net->name != NAME_SINGLE),
                 TTUP_EFORMAT, "uplift blob: variant %d / time rotation %d is none that get_model builds", hdr[6], hdr[7]);
    TTUP_REQUIRE(net->D > 0 && net->D % 32 == 0 && net->D <= 256 && net->heads > 0 && net->D % net->heads == 0, TTUP_EFORMAT,
                 "uplift blob: dim %d / heads %d unsupported", net->D, net->heads);
    net->hd = net->D / net->heads;
    TTUP_REQUIRE(net->hd == 8 || net->hd == 16 || net->hd == 24 || net->hd == 32, TTUP_EFORMAT, "uplift blob: head_dim %d unsupported", net->hd);
    TTUP_REQUIRE(net->n_table == 13 && n_pos >= 0 && n_first >= 0 && n_second >= 0 && n_pos + n_first + n_second <= 64, TTUP_EFORMAT, "uplift blob: bad layer counts");
    TTUP_REQUIRE((n_pos > 0) == (net->mode == MODE_DYNAMIC) && n_first > 0 && (n_second > 0) == (net->name != NAME_SINGLE), TTUP_EFORMAT,
                 "uplift blob: layer counts %d/%d/%d do not fit variant %d", n_pos, n_first, n_second, hdr[6]);
    net->max_batch = max_batch; net->max_len = max_len;
    net->pos_layers.resize(n_pos); net->layers.resize(n_first); net->second.resize(n_second);
    return TTUP_OK;
}

// the weight records in blob order (arch.uplift_variant_schema), then what is derived from them: the stage tables, the table tokens' RoPE
int load_weights(ttup_uplift* net, Reader r) {
    int rc;
    const int D = net->D;
    std::vector<float> inv_freq, plain;
    TTUP_REQUIRE(r.take(&inv_freq, net->hd / 2), TTUP_EFORMAT, "uplift blob: bad inv_freq record");
    if ((rc = dev_copy(net, inv_freq, &net->inv_freq_dev))) return rc;
    if (net->name == NAME_CONNECT && net->mode == MODE_DYNAMIC) r.keep = &plain;
    if ((rc = make_vec(net, r, D, &net->cls_dev))) return rc;
    if (net->mode == MODE_STACKED || net->mode == MODE_ORIGINAL) {
        if ((rc = make_linear_t(net, r, D, 2 + net->n_table * (net->mode == MODE_STACKED ? 3 : 2), &net->stacked_wt, &net->stacked_b))) return rc;
        if ((rc = make_linear(net, r, D, D, true, &net->ball_embed.fc2))) return rc;
    } else if ((rc = make_mlp2(net, r, 2, &net->ball_embed))) return rc;
    if (net->mode == MODE_DYNAMIC && (rc = make_mlp2(net, r, 2, &net->table_embed))) return rc;
    for (auto& L : net->pos_layers) if ((rc = make_layer(net, r, &L))) return rc;
    for (auto& L : net->layers) if ((rc = make_layer(net, r, &L))) return rc;
    if ((rc = make_head(net, r, &net->position_head))) return rc;
    if (net->name == NAME_MULTI) {
        if ((rc = make_linear_t(net, r, D, 3, &net->embed_w1t, &net->embed_b1))) return rc;
        if ((rc = make_linear_t(net, r, D, D, &net->embed_w2t, &net->embed_b2))) return rc;
    }
    for (auto& L : net->second) if ((rc = make_layer(net, r, &L))) return rc;
    if ((rc = make_head(net, r, &net->rotation_head))) return rc;
    TTUP_REQUIRE(r.left == 0, TTUP_EFORMAT, "uplift blob: %zu trailing bytes", r.left);
    if (r.keep) {
        if ((rc = dev_copy(net, plain, &net->plain))) return rc;
        net->plain_floats = (long long)plain.size();
    }
    make_stage(net, net->pos_layers, &net->stage_pos);
    make_stage(net, net->layers, &net->stage_first);
    make_stage(net, net->second, &net->stage_second);
    std::vector<float> tt(net->n_table);
    for (int n = 0; n < net->n_table; ++n) tt[n] = (float)n / 100.0f;       // arange(13) / (MAX_FPS/5), model.py:367
    if ((rc = dev_copy(net, tt, &net->table_times_dev))) return rc;
    if ((rc = dev_alloc(net, {{(void**)&net->table_rope, (size_t)net->n_table * net->hd}}))) return rc;
    const long long n = (long long)net->n_table * (net->hd / 2);
    // ('new' turns table token n by index round(n/100 / 0.002) = 5n, 'old' by n itself)
    if (net->rot_old) return launch_1d(rope_index_kernel, n, 0, net->inv_freq_dev, net->table_rope, net->hd / 2, n);
    return launch_1d(rope_table_kernel, n, 0, net->table_times_dev, net->inv_freq_dev, net->table_rope, net->hd / 2, n);
}

// scratch: chunk of trajectories such that the table stage holds at most ~2M tokens (7 GB of fp32 scratch at D=128)
int alloc_scratch(ttup_uplift* net) {
    const size_t D = net->D, NT = net->n_table, hd = net->hd;
    const long long per_traj = (long long)net->max_len * (net->n_table + 1);
    long long fit = (2048 * 1024) / per_traj;
    if (fit < 1) fit = 1;
    if (fit > net->max_batch) fit = net->max_batch;
    net->chunk = (int)fit;
    const size_t chunk = (size_t)fit, tokmax = chunk * per_traj, bt = chunk * (net->max_len + 1);
    // h1 holds the hidden rows of BOTH embeddings in turn: a ball token per step, then 13 table tokens per trajectory -- more rows than
    // steps when max_len < 12 (it used to be sized by the steps alone: the table embedding of a short model wrote past its end)
    const size_t h1_rows = bt > chunk * NT ? bt : chunk * NT;
    const size_t index_rows = net->rot_old ? (size_t)net->max_len + 64 : 0;          // (the attention kernels' padded key tiles stay inside the table)
    if (int rc = dev_alloc(net, {{(void**)&net->x, tokmax * D}, {(void**)&net->qkv, tokmax * 3 * D}, {(void**)&net->att, tokmax * D},
                                 {(void**)&net->hid, tokmax * D}, {(void**)&net->x2, tokmax * D}, {(void**)&net->tok, bt * D},
                                 {(void**)&net->h1, h1_rows * D}, {(void**)&net->ttok, chunk * NT * D}, {(void**)&net->m1, bt},
                                 {(void**)&net->m2, bt}, {(void**)&net->tmask, chunk * (NT + 1)}, {(void**)&net->txy, chunk * NT * 2},
                                 {(void**)&net->rope, bt * hd}, {(void**)&net->rope_index, index_rows * hd},
                                 {(void**)&net->pos_rows, net->name == NAME_SINGLE ? bt * 3 : 0}, {(void**)&net->flags_dev, 4}}))
        return rc;
    if (!net->rot_old) return TTUP_OK;
    const long long n = (long long)index_rows * (net->hd / 2);
    return launch_1d(rope_index_kernel, n, 0, net->inv_freq_dev, net->rope_index, net->hd / 2, n);
}

// graph path: batches of up to GRAPH_TOKENS ball tokens (batch * len)
int alloc_graph_buffers(ttup_uplift* net) {
    const long long GRAPH_TOKENS = 1024, all = (long long)net->max_batch * net->max_len;
    long long gt = all < GRAPH_TOKENS ? all : GRAPH_TOKENS;
    if (gt < net->max_len) gt = net->max_len;          // at least one trajectory of the longest length
    net->graph_tokens = gt;
    net->graphs_off = env_set("TTUP_UPLIFT_NO_GRAPH");
    const size_t nb = (size_t)(gt > net->max_batch ? net->max_batch : gt);          // trajectories a graph call can hold (len >= 1)
    return dev_alloc(net, {{(void**)&net->g_ball, (size_t)gt * 2}, {(void**)&net->g_table, nb * net->n_table * 3}, {(void**)&net->g_mask, (size_t)gt},
                           {(void**)&net->g_times, (size_t)gt}, {(void**)&net->g_rot, nb * 3}, {(void**)&net->g_pos, (size_t)gt * 3}});
}

// The small-batch path (uplift_net.h): the first call with a shape runs eagerly (and sets every kernel's attributes), the second captures
// forward_chunk on the handle's own buffers, every later one replays.  *done = false: the caller runs this call eagerly.
int forward_graph(ttup_uplift* net, const float* ball_dev, const float* table_dev, const float* mask_dev, const float* times_dev, int batch, int len,
                  float* rot_dev, float* pos_dev, hipStream_t st, bool* done) {
    *done = false;
    // (a length no attention kernel serves would fail inside the capture and be taken for a runtime that cannot capture)
    TTUP_REQUIRE(len + 1 <= max_attention_seq(net), TTUP_EINVAL, "uplift graph: sequence length %d + 1 exceeds the %d tokens the attention kernels serve", len, max_attention_seq(net));
    ttup_uplift::GraphEntry& ge = net->graphs[{batch, len}];
    if (!ge.exec && ge.seen++ == 0) return TTUP_OK;          // first call with this shape
    const size_t bt = (size_t)batch * len;
    TTUP_HIP_CHECK(hipMemcpyAsync(net->g_ball, ball_dev, bt * 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
    TTUP_HIP_CHECK(hipMemcpyAsync(net->g_table, table_dev, (size_t)batch * net->n_table * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    TTUP_HIP_CHECK(hipMemcpyAsync(net->g_mask, mask_dev, bt * sizeof(float), hipMemcpyDeviceToDevice, st));
    TTUP_HIP_CHECK(hipMemcpyAsync(net->g_times, times_dev, bt * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (!ge.exec) {
        hipGraph_t graph = nullptr;
        bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            const int rc = forward_chunk(net, net->g_ball, net->g_table, net->g_mask, net->g_times, batch, len, net->g_rot, net->g_pos, st);
            ok = hipStreamEndCapture(st, &graph) == hipSuccess && rc == TTUP_OK && graph;
        }
        if (ok) ok = hipGraphInstantiate(&ge.exec, graph, nullptr, nullptr, 0) == hipSuccess;
        if (graph) (void)hipGraphDestroy(graph);
        if (!ok) {          // this runtime cannot capture the forward: eager from now on
            if (env_set("TTUP_DEBUG")) fprintf(stderr, "ttup_uplift: graph capture failed (%s): eager from now on\n", hipGetErrorString(hipGetLastError()));
            (void)hipGetLastError(); ge.exec = nullptr; net->graphs_off = true;
            return TTUP_OK;
        }
    }
    TTUP_HIP_CHECK(hipGraphLaunch(ge.exec, st));
    net->graph_replays++;
    TTUP_HIP_CHECK(hipMemcpyAsync(rot_dev, net->g_rot, (size_t)batch * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    TTUP_HIP_CHECK(hipMemcpyAsync(pos_dev, net->g_pos, bt * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    *done = true;
    return TTUP_OK;
}

}  // namespace

extern "C" int ttup_uplift_create(const void* blob, size_t blob_bytes, int max_batch, int max_len, ttup_uplift** out) {
    TTUP_REQUIRE(blob && out, TTUP_EINVAL, "ttup_uplift_create: null pointer");
    TTUP_REQUIRE(max_batch > 0 && max_len > 0, TTUP_EINVAL, "ttup_uplift_create: max_batch and max_len must be positive");
    TTUP_REQUIRE(blob_bytes >= 40 && memcmp(blob, "TTUPUPL1", 8) == 0, TTUP_EFORMAT, "uplift blob: bad magic");
    int rc, ndev = 0;
    TTUP_HIP_CHECK(hipGetDeviceCount(&ndev));
    TTUP_REQUIRE(ndev > 0, TTUP_EHIP, "ttup_uplift_create: no HIP device");
    std::unique_ptr<ttup_uplift> net(new ttup_uplift);
    if ((rc = parse_header(blob, max_batch, max_len, net.get()))) return rc;
    if ((rc = load_weights(net.get(), Reader{(const char*)blob + 40, blob_bytes - 40}))) return rc;
    if ((rc = alloc_scratch(net.get()))) return rc;
    if ((rc = alloc_graph_buffers(net.get()))) return rc;
    TTUP_HIP_CHECK(hipDeviceSynchronize());
    *out = net.release();
    return TTUP_OK;
}

extern "C" void ttup_uplift_destroy(ttup_uplift* net) {
    if (!net) return;
    (void)hipDeviceSynchronize();
    delete net;
}

extern "C" int ttup_uplift_forward(ttup_uplift* net, const float* ball_dev, const float* table_dev, const float* mask_dev,
                                   const float* times_dev, int batch, int len, float* rot_dev, float* pos_dev, int check_mask, void* stream) {
    TTUP_REQUIRE(net && ball_dev && table_dev && mask_dev && times_dev && rot_dev && pos_dev, TTUP_EINVAL, "ttup_uplift_forward: null pointer");
    TTUP_REQUIRE(batch >= 0 && batch <= net->max_batch, TTUP_EINVAL, "ttup_uplift_forward: batch %d outside [0,%d]", batch, net->max_batch);
    TTUP_REQUIRE(len > 0 && len <= net->max_len, TTUP_EINVAL, "ttup_uplift_forward: sequence length %d outside [1,%d]", len, net->max_len);
    // every variant ends in a stage of cls + len tokens: refused here, before anything is launched or captured
    TTUP_REQUIRE(len + 1 <= max_attention_seq(net), TTUP_EINVAL, "ttup_uplift_forward: sequence length %d too long: with the cls token it exceeds the %d tokens this model's attention kernels serve",
                 len, max_attention_seq(net));
    TTUP_REQUIRE(!net->trained, TTUP_ESTALE, "ttup_uplift_forward: this handle's weights were trained, its packed weights are stale: build an inference model from the trainer");
    hipStream_t st = (hipStream_t)stream;
    if (batch == 0) return TTUP_OK;
    TTUP_HIP_CHECK(hipMemsetAsync(net->flags_dev, 0, sizeof(int), st));
    const long long cap = net->chunk;      // scratch is sized for `chunk` trajectories of max_len tokens
    bool done = false;
    if (!net->graphs_off && st != nullptr && batch <= cap && (long long)batch * len <= net->graph_tokens &&          // (stream 0 is never captured)
        (net->graphs.size() < 32 || net->graphs.count({batch, len})))          // (at most 32 shapes are kept)
        if (int rc = forward_graph(net, ball_dev, table_dev, mask_dev, times_dev, batch, len, rot_dev, pos_dev, st, &done)) return rc;
    for (int b0 = 0; b0 < batch && !done; b0 += (int)cap) {
        const int nb = batch - b0 < cap ? batch - b0 : (int)cap;
        const int rc = forward_chunk(net, ball_dev + (size_t)b0 * len * 2, table_dev + (size_t)b0 * net->n_table * 3, mask_dev + (size_t)b0 * len,
                                     times_dev + (size_t)b0 * len, nb, len, rot_dev + (size_t)b0 * 3, pos_dev + (size_t)b0 * len * 3, st);
        if (rc) return rc;
    }
    if (check_mask) {
        int flags = 0;
        TTUP_HIP_CHECK(hipMemcpyAsync(&flags, net->flags_dev, sizeof(int), hipMemcpyDeviceToHost, st));
        TTUP_HIP_CHECK(hipStreamSynchronize(st));
        // reference: mask.min()==0 and mask.max()==1, else ValueError (model.py:541-546); the already-additive
        // {-1e9,0} format of the elif branch is not accepted here
        TTUP_REQUIRE(flags == 3, TTUP_EMASK, "wrong format for masks. Should be 0, 1 or -1e9, 0.");
    }
    return TTUP_OK;
}

// how the small-batch path is doing: out_host[0] = captured graphs, [1] = 1 when capturing failed on this runtime (eager from then
// on) or was switched off (TTUP_UPLIFT_NO_GRAPH), [2] = forwards served by a graph replay
extern "C" int ttup_uplift_graph_info(ttup_uplift* net, int* out_host3) {
    TTUP_REQUIRE(net && out_host3, TTUP_EINVAL, "ttup_uplift_graph_info: null pointer");
    int n = 0;
    for (auto& kv : net->graphs) n += kv.second.exec != nullptr;
    out_host3[0] = n; out_host3[1] = net->graphs_off ? 1 : 0; out_host3[2] = (int)net->graph_replays;
    return TTUP_OK;
}

// stage_x3_kernel launches issued (or captured into a graph) so far: all layers of a stage in one launch, small batches only
extern "C" int ttup_uplift_stage_info(ttup_uplift* net, long long* out_host) {
    TTUP_REQUIRE(net && out_host, TTUP_EINVAL, "ttup_uplift_stage_info: null pointer");
    *out_host = net->stage_launches;
    return TTUP_OK;
}

extern "C" int ttup_transform_rotationaxes(const float* rot_dev, const float* pos_dev, int batch, int len, float* out_dev, void* stream) {
    TTUP_REQUIRE(rot_dev && pos_dev && out_dev, TTUP_EINVAL, "ttup_transform_rotationaxes: null pointer");
    TTUP_REQUIRE(batch >= 0 && len >= 2, TTUP_EINVAL, "ttup_transform_rotationaxes: need at least two positions");
    if (batch == 0) return TTUP_OK;
    hipLaunchKernelGGL(rotationaxes_kernel, dim3(cdiv(batch, 64)), dim3(64), 0, (hipStream_t)stream, rot_dev, pos_dev, batch, len, out_dev);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

#include "no_packed_fp32_end.h"
