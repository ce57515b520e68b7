// Certified argmax: the production CNN runs in bf16, the reference (balldetection/models/wasb.py, fp32) takes
// `torch.argmax` of the fp32 heatmap (balldetection/helper_balldetection.py:50).  north_star asks for bit-exact argmax
// indices, and bf16 rounding (|error| <= eps, a bound the caller calibrates against the fp32 path) can reorder pixels
// whose fp32 values are closer than 2*eps.  So the index is made exact by construction instead of by luck:
//
//   1. scan      every pixel whose bf16 value is within 2*eps of the bf16 maximum is a candidate -- no other pixel can be
//                the fp32 argmax.  One streaming pass over the fp32-stored heatmap (3.6 MB per frame, HBM-bound).
//   2. plan      one candidate: certified as is.  Several: they are grouped into crops of `Hc x Wc` pixels whose origin is a
//                multiple of 8 (the three stride-2 levels and the nearest-neighbour upsampling then sample exactly as in the
//                full frame).  A heatmap pixel depends on the inputs within R = 72 pixels (measured receptive-field radius 71),
//                so every candidate at least R inside its crop -- or next to a true image border, where the crop's zero padding
//                IS the frame's -- gets bit for bit the value the fp32 path computes on the whole frame.
//   3. crops     the selected windows are pre-processed again in fp32 from the uint8 frames and run through the SAME fp32
//                graph (csrc/conv_f32.hip, the fp32 matrix pipe) as a small batch; everything is sized on the device
//                (`n_active`), nothing synchronises with the host.
//   4. resolve   the candidate with the largest fp32 value (ties -> smaller index, like torch.argmax) becomes the index,
//                and its 3x3 window is taken from the fp32 crop, so the sub-pixel fit also sees fp32 values.
// Heatmaps whose candidates overflow the budget (more than K candidates, more than `maxc` crops, crop list full) are
// flagged 2 in `status`; the caller decides (the Python shim re-runs those frames on the full-frame fp32 handle).  An audit crop
// that finds no room is dropped instead: its heatmap has one candidate and stays status 0, whatever the audit phase.
// The integer decisions of the plan -- status values, counters, crop record, crop geometry, sizing -- are csrc/certify_plan.h, which
// compiles without a device and is checked on the CPU (tests/test_certify_plan_host.py); this file holds the kernels of the four
// steps, cert_begin / scan / finish / free and the handle's certify ABI.
#include "wasb_net.h"

namespace ttup {

namespace {

struct Best { float v; long long i; };
__device__ __forceinline__ bool better(float v, long long i, float bv, long long bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

// ---- 1. candidates of each heatmap of a micro-batch: heat (n_maps, hw) fp32, argmax (n_maps)
__global__ __launch_bounds__(256) void cert_scan_kernel(const float* __restrict__ heat, const long long* __restrict__ argmax, long long hw,
                                                        float two_eps, int K, int* __restrict__ cand_idx, int* __restrict__ cand_cnt,
                                                        float* __restrict__ cand_bf, float guard_two_eps, int* __restrict__ guard_cnt) {
    const int map = blockIdx.y;
    const float* h = heat + (size_t)map * hw;
    const float hmax = h[argmax[map]];
    if (hmax != hmax) return;                 // NaN maximum: torch.argmax returns the first NaN, which the bf16 pass already did
    const float thr = hmax - two_eps;
    // guard band: pixels just below the candidate band, down to 2 * (GUARD * eps).  A heatmap without any keeps its candidate set
    // -- and with it its certified result -- when eps is widened by up to the factor GUARD (the shim then re-runs only the others)
    const float gthr = guard_cnt ? hmax - guard_two_eps : thr;
    const long long quads = hw / 4;
    const float4* h4 = (const float4*)h;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long long)gridDim.x * 256) {
        const float4 v = h4[q];
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e[k] >= thr) {
                const int slot = atomicAdd(&cand_cnt[map], 1);
                if (slot < K) { cand_idx[(size_t)map * K + slot] = (int)(q * 4 + k); cand_bf[(size_t)map * K + slot] = e[k]; }
            } else if (e[k] >= gthr) atomicAdd(&guard_cnt[map], 1);
    }
}

struct PlanArgs {
    int* cand_idx; int* cand_cnt; int* cand_crop; CropRec* crop_rec; int* n_crops; int* status; unsigned long long* stats; float* cand_bf;
    int K, maxc, max_crops, H, W, Hc, Wc, R, frame0, exact;
    int C, maxf;          // heatmap channels per frame (1 ball, 13 table keypoints) and crops a frame may use in all
    int audit_mod, audit_phase;          // audit crops (ttup_wasb_certify_audit_crops): 0 = off
    int small;                           // class-2 crops (conv.h Roi): valid core positions R + 1 .. R + small of a crop whose candidates all fit there; 0 = off
    const int* guard_cnt;
    float* margin;
};

__device__ __forceinline__ void bump(unsigned long long* stats, CertStat k, unsigned long long n = 1ull) { atomicAdd(&stats[k], n); }
// (lane 0) a heatmap's final status with its counters: a certified single candidate / not certified for the reason `why`
__device__ __forceinline__ void set_single(const PlanArgs& a, int map, int gbit) { a.status[map] = CERT_SINGLE | gbit; bump(a.stats, CS_single); }
__device__ __forceinline__ void set_not_certified(const PlanArgs& a, int map, int gbit, CertStat why) {
    a.status[map] = CERT_NOT_CERTIFIED | gbit; bump(a.stats, CS_not_certified); bump(a.stats, why);
}

// ---- 2. one workgroup (one wave) per FRAME, its C heatmaps (channels) in turn: the wave sorts a heatmap's candidates by index (the
// scan appends in arbitrary order; a rank sort: every lane counts the smaller indices of its elements), lane 0 opens the crops
// (csrc/certify_plan.h cert_open_crop).  The crops belong to the frame: a crop is one fp32 pass over a window of the frame and yields
// ALL C channels there, so the keypoint heatmaps of the table detector share crops (the ball detector has C = 1).  K is sized for the
// flat top of a wide saturated blob (a few hundred equal pixels inside one crop core).
__global__ __launch_bounds__(64) void cert_plan_kernel(PlanArgs a) {
    // The whole wave works on the assignment: with one lane walking the sorted list in GLOBAL memory -- a dependent load per candidate,
    // a read-modify-write per candidate for the final crop ids -- it took 19 us on average and up to 63 us per micro-batch on varied
    // content; 12 / 26 us in this form.  (The 0.18 ms average / 0.7 ms maximum this kernel shows in the two-lane kernel trace is NOT
    // its own time: its eight small workgroups wait for a slot while the other lane's persistent kernels -- two 256-VGPR waves per
    // SIMD on every CU -- run to their end; the trace counts from the dispatch.)  Same decisions as the serial walk: a candidate goes
    // to the FIRST crop of the frame's list whose core holds it; the first candidate (in index order) that no crop holds opens a new one.
    __shared__ int s_idx[CERT_MAX_K];            // as scanned, then the crop slot of every sorted candidate
    __shared__ float s_bf[CERT_MAX_K];
    __shared__ int s_sorted[CERT_MAX_K];
    __shared__ int my_y0[CERT_MAX_FRAME_CROPS], my_x0[CERT_MAX_FRAME_CROPS], my_small[CERT_MAX_FRAME_CROPS];
    __shared__ int n_my_s, s_base;
    constexpr int PER = CERT_MAX_K / 64;         // candidates per lane
    const int lane = threadIdx.x;
    const int frame = a.frame0 + blockIdx.x;
    if (lane == 0) n_my_s = 0;
    __syncthreads();
    for (int ch = 0; ch < a.C; ++ch) {
        const int map = frame * a.C + ch;
        const int cnt = a.cand_cnt[map];
        const int gbit = a.guard_cnt[map] > 0 ? CERT_GUARD : 0;
        if (lane == 0) { bump(a.stats, CS_heatmaps); a.margin[map] = __int_as_float(0x7f800000); }
        // exact-window mode: a single candidate still gets its fp32 crop (the index is certain, the 3x3 window becomes fp32 too).
        // Audit crops: so does the single candidate of ONE channel of every audit_mod-th frame -- its crop reports |bf16 - fp32| at the
        // winner like every crop does (cand_bf / CS_max_candidate_err), which is how a frame whose error exceeds eps WITHOUT producing
        // a near-tie gets noticed between two strip audits
        const bool audit_pick = cert_audit_pick(a.audit_mod, a.audit_phase, cnt, frame, ch, a.C);
        if (cnt <= 0 || (cnt == 1 && !a.exact && !audit_pick)) { if (lane == 0) set_single(a, map, gbit); continue; }
        if (cnt > a.K) { if (lane == 0) set_not_certified(a, map, gbit, CS_over_candidates); continue; }
        int* ci = a.cand_idx + (size_t)map * a.K;
        float* cb = a.cand_bf + (size_t)map * a.K;
        __syncthreads();                                          // (the previous channel is done with the shared lists)
        for (int i = lane; i < cnt; i += 64) { s_idx[i] = ci[i]; s_bf[i] = cb[i]; }
        __syncthreads();
        for (int i = lane; i < cnt; i += 64) {
            const int v = s_idx[i];
            int rank = 0;
            for (int j = 0; j < cnt; ++j) rank += s_idx[j] < v;          // pixel indices are distinct: ranks are a permutation
            ci[rank] = v; cb[rank] = s_bf[i]; s_sorted[rank] = v;
        }
        __syncthreads();
        // the lane's candidates lane, lane + 64, ...: position and the slot of the first crop that holds them (-1: none yet)
        int cy[PER], cx[PER], found[PER];
#pragma unroll
        for (int m = 0; m < PER; ++m) {
            const int i = lane + 64 * m;
            const int v = i < cnt ? s_sorted[i] : 0;
            cy[m] = v / a.W; cx[m] = v - cy[m] * a.W; found[m] = -1;
        }
        // crops the frame has so far (from its earlier channels) are tried first; new ones are added behind them and dropped again
        // if this heatmap turns out to need more than its budget
        int n_my = n_my_s;
        const int n_before = n_my;
        bool over = false;
        int c_from = 0;                                           // crops [c_from, n_my) have not been tried on the uncovered candidates yet
        while (true) {
            for (int c = c_from; c < n_my; ++c) {
                int ylo, yhi, xlo, xhi;
                cert_core_range(my_y0[c], a.Hc, a.H, a.R, my_small[c], ylo, yhi);
                cert_core_range(my_x0[c], a.Wc, a.W, a.R, my_small[c], xlo, xhi);
#pragma unroll
                for (int m = 0; m < PER; ++m)
                    if (found[m] < 0 && cy[m] >= ylo && cy[m] < yhi && cx[m] >= xlo && cx[m] < xhi) found[m] = c;
            }
            c_from = n_my;
            int first = -1;                                       // the first candidate (index order) that no crop holds
#pragma unroll
            for (int m = 0; m < PER; ++m) {
                const unsigned long long unc = __builtin_amdgcn_ballot_w64(lane + 64 * m < cnt && found[m] < 0);
                if (first < 0 && unc) first = 64 * m + __builtin_ctzll(unc);
            }
            if (first < 0) break;
            if (n_my - n_before >= a.maxc || n_my >= a.maxf) { over = true; break; }
            if (lane == 0) {          // (the new crop's core holds candidate `first`, so every round covers one more: certify_plan.h)
                const NewCrop nc = cert_open_crop(s_sorted, cnt, first, a.H, a.W, a.Hc, a.Wc, a.R, a.small);
                my_y0[n_my] = nc.y0; my_x0[n_my] = nc.x0; my_small[n_my] = nc.small;
            }
            ++n_my;
            __syncthreads();
        }
        if (over && audit_pick && !a.exact) { if (lane == 0) set_single(a, map, gbit); continue; }          // (no room in the frame for the audit: still a certified single candidate)
        if (over) { if (lane == 0) set_not_certified(a, map, gbit, CS_over_crops_per_map); continue; }          // (n_my_s keeps the list without this heatmap's new crops)
#pragma unroll
        for (int m = 0; m < PER; ++m)
            if (lane + 64 * m < cnt) a.cand_crop[(size_t)map * a.K + lane + 64 * m] = found[m];          // slot in the frame's list for now
        __syncthreads();                                          // (every lane has read n_my_s)
        if (lane == 0) { n_my_s = n_my; a.status[map] = CERT_PENDING | gbit | ((audit_pick && !a.exact) ? CERT_AUDIT_ONLY : 0); }
    }
    __syncthreads();
    const int n_my = n_my_s;
    if (n_my == 0) return;
    if (lane == 0) {
        const int base = atomicAdd(a.n_crops, n_my);
        s_base = base;
        for (int c = 0; c < n_my && base + c < a.max_crops; ++c)          // (records also for a list that fills up half way: the slots are run)
            a.crop_rec[base + c] = CropRec{frame, my_y0[c], my_x0[c], my_small[c] > 0 ? 1 : 0};
        if (!(base + n_my > a.max_crops)) {
            bump(a.stats, CS_crops, (unsigned long long)n_my);
            int ns = 0;
            for (int c = 0; c < n_my; ++c) ns += my_small[c] > 0;
            if (ns) bump(a.stats, CS_small_crops, (unsigned long long)ns);
        }
    }
    __threadfence_block();
    __syncthreads();
    const int base = s_base;
    const bool full = base + n_my > a.max_crops;                          // crop list full: the frame's heatmaps stay uncertified
    for (int ch = 0; ch < a.C; ++ch) {
        const int map = frame * a.C + ch;
        const int st = a.status[map];          // (written by lane 0 of this workgroup above: visible after the barrier)
        if (!(st & CERT_PENDING)) continue;
        const int gbit = st & CERT_GUARD, abit = st & CERT_AUDIT_ONLY;
        if (full && abit) { if (lane == 0) set_single(a, map, gbit); continue; }          // (no room for the audit: still a certified single candidate)
        if (full) { if (lane == 0) set_not_certified(a, map, gbit, CS_over_crop_list); continue; }
        const int cnt = a.cand_cnt[map];
        for (int k = lane; k < cnt; k += 64) a.cand_crop[(size_t)map * a.K + k] += base;
        if (lane == 0) {
            a.status[map] = CERT_RESOLVED | gbit | abit;
            if (cnt == 1) bump(a.stats, CS_exact_singles);          // (counted where the single candidate's crop is kept)
            if (abit) bump(a.stats, CS_single);                     // an audit-only heatmap returns as a single candidate (cert_resolve_kernel)
            else { bump(a.stats, CS_resolved); bump(a.stats, CS_candidates, (unsigned long long)cnt); }
        }
    }
}

__global__ void cert_active_kernel(const int* n_crops, int* n_active, int CH, int nchunks, int max_crops, const CropRec* crop_rec, int* roi_flag,
                                   int H, int W, int Hc, int Wc) {
    const int c = threadIdx.x;
    if (c >= nchunks) return;
    int n = *n_crops;
    n = n > max_crops ? max_crops : n;
    int v = n - c * CH;
    v = v < 0 ? 0 : (v > CH ? CH : v);
    n_active[c] = v;
    // one flag per crop; the kernels skip the tiles / pixels outside an op's region for the flagged samples only
    for (int j = 0; j < v; ++j) roi_flag[c * CH + j] = cert_roi_class(crop_rec[c * CH + j], H, W, Hc, Wc);
}

// crop windows of a caller-supplied fp32 NCHW input (the `forward(x)` entry): -> fp32 NHWC16
__global__ void cert_gather_kernel(const float* __restrict__ x, int in_ch, int H, int W, const CropRec* __restrict__ crops, int crop0,
                                   const int* __restrict__ n_active, int Hc, int Wc, float* __restrict__ out, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cx = (int)(i % Wc);
    long long p = i / Wc;
    const int cy = (int)(p % Hc);
    const int j = (int)(p / Hc);
    if (j >= *n_active) return;
    const CropRec rec = crops[crop0 + j];
    const size_t hw = (size_t)H * W, pix = (size_t)(rec.y0 + cy) * W + rec.x0 + cx;
    float* o = out + (size_t)i * 16;
    for (int c = 0; c < 16; ++c) o[c] = c < in_ch ? x[((size_t)rec.frame * in_ch + c) * hw + pix] : 0.f;
}

// ---- 4a. fp32 value and 3x3 window of every candidate whose crop is in this chunk
__global__ void cert_lookup_kernel(const int* __restrict__ cand_idx, const int* __restrict__ cand_cnt, const int* __restrict__ cand_crop,
                                   const int* __restrict__ status, const CropRec* __restrict__ crop_rec, const float* __restrict__ crop_heat,
                                   int K, int H, int W, int Hc, int Wc, int crop0, int CH, int n_maps, float* __restrict__ cand_val, float* __restrict__ cand_win,
                                   const float* __restrict__ cand_bf, unsigned long long* __restrict__ stats, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_maps * K) return;
    const int map = i / K, k = i % K;
    if ((status[map] & CERT_STATUS_MASK) != CERT_RESOLVED || k >= cand_cnt[map]) return;
    const int id = cand_crop[i];
    if (id < crop0 || id >= crop0 + CH) return;
    const CropRec rec = crop_rec[id];
    const int gy = cand_idx[i] / W, gx = cand_idx[i] % W;
    const float* h = crop_heat + ((size_t)(id - crop0) * C + map % C) * Hc * Wc;          // crop_heat (CH, C, Hc, Wc)
    const float vf = h[(size_t)(gy - rec.y0) * Wc + (gx - rec.x0)];
    cand_val[i] = vf;
    // audit of the error bound: |bf16 - fp32| at every candidate comes for free here; the running maximum sits in its counter (the
    // bits of a non-negative float order like the unsigned integer they spell)
    const float err = fabsf(cand_bf[i] - vf);
    if (err == err) atomicMax(&stats[CS_max_candidate_err], (unsigned long long)__float_as_uint(err));
    for (int t = 0; t < 9; ++t) {
        const int y = gy + t / 3 - 1, x = gx + t % 3 - 1;
        float v = 0.f;                        // zero padding outside the IMAGE (helper_balldetection.py:55-64)
        if (y >= 0 && y < H && x >= 0 && x < W) v = h[(size_t)(y - rec.y0) * Wc + (x - rec.x0)];
        cand_win[(size_t)i * 9 + t] = v;
    }
}

// ---- 4b. the fp32 winner of every heatmap that needed crops
__global__ void cert_resolve_kernel(const int* __restrict__ cand_idx, const int* __restrict__ cand_cnt, int* __restrict__ status,
                                    const float* __restrict__ cand_val, const float* __restrict__ cand_win, int K, int n_maps,
                                    long long* __restrict__ argmax, float* __restrict__ win, float* __restrict__ margin) {
    const int map = blockIdx.x * blockDim.x + threadIdx.x;
    if (map >= n_maps || (status[map] & CERT_STATUS_MASK) != CERT_RESOLVED) return;
    // an audit crop has left its |bf16 - fp32| in the counters (cert_lookup_kernel): the heatmap's result is what the bf16 path returned,
    // whatever frames an audit happens to look at (outputs do not depend on the audit phase); status back to "single candidate"
    if (status[map] & CERT_AUDIT_ONLY) { status[map] = CERT_SINGLE | (status[map] & CERT_GUARD); return; }
    const int cnt = cand_cnt[map];
    float bv = cand_val[(size_t)map * K];
    long long bi = cand_idx[(size_t)map * K];
    int bk = 0;
    float second = -__int_as_float(0x7f800000);
    for (int k = 1; k < cnt; ++k) {
        const float v = cand_val[(size_t)map * K + k];
        const long long i = cand_idx[(size_t)map * K + k];
        if (better(v, i, bv, bi)) { second = bv; bv = v; bi = i; bk = k; }
        else if (v > second) second = v;
    }
    argmax[map] = bi;
    margin[map] = bv - second;          // how far the fp32 winner is ahead of the best other candidate (measurement: "reference-ambiguous" share)
    for (int t = 0; t < 9; ++t) win[(size_t)map * 9 + t] = cand_win[((size_t)map * K + bk) * 9 + t];
}

// the scan of n_maps heatmaps of hw pixels each (guard_cnt may be null: no guard band)
int launch_scan(const float* heat, const long long* argmax, int n_maps, long long hw, float two_eps, int K, int* cand_idx, int* cand_cnt,
                float* cand_bf, float guard_two_eps, int* guard_cnt, hipStream_t st) {
    int nblk = (int)(hw / 4 / 256 / 8);           // 8 float4 per thread
    nblk = nblk < 1 ? 1 : (nblk > 256 ? 256 : nblk);
    hipLaunchKernelGGL(cert_scan_kernel, dim3(nblk, n_maps), dim3(256), 0, st, heat, argmax, hw, two_eps, K, cand_idx, cand_cnt, cand_bf, guard_two_eps, guard_cnt);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

// The per-call arrays of a slot in ONE allocation, each at a 256-byte offset.  base = 0 only measures: returns the bytes needed.
// The arrays that cert_begin zeroes come first and lie back to back: cand_cnt, guard_cnt, status (nb each), n_crops (1).
size_t carve_slot(CertState::Slot& sl, uintptr_t base, size_t nb, int K, int max_crops, int nchunks) {
    size_t off = 0;
    auto take = [&](auto*& p, size_t n) {
        p = (decltype(+p))(base + off);
        off += (n * sizeof(*p) + 255) & ~(size_t)255;
    };
    take(sl.cand_cnt, 3 * nb + 1);
    sl.guard_cnt = sl.cand_cnt + nb; sl.status = sl.guard_cnt + nb; sl.n_crops = sl.status + nb;
    take(sl.cand_idx, nb * K); take(sl.cand_crop, nb * K); take(sl.cand_val, nb * K); take(sl.cand_bf, nb * K); take(sl.cand_win, nb * K * 9);
    take(sl.crop_rec, (size_t)max_crops); take(sl.n_active, (size_t)nchunks); take(sl.roi_flag, (size_t)max_crops); take(sl.margin, nb);
    return off;
}
size_t slot_zeroed_bytes(const ttup_wasb* net) { return (3 * (size_t)net->max_batch * net->n_out + 1) * sizeof(int); }

// The experiment knobs, read once per process
const CertKnobs& cert_knobs() {
    static const CertKnobs knobs = [] {
        CertKnobs k;
        k.list = (int)env_ll("TTUP_CERT_LIST", 0);
        k.ch = (int)env_ll("TTUP_CERT_CH", 0);
        k.no_small = env_ll("TTUP_CERT_SMALL", 1) == 0;
        k.no_cone = env_set("TTUP_NO_CONE") || env_set("TTUP_F32_EXACT") || env_set("TTUP_F32_DIRECT");
        return k;
    }();
    return knobs;
}

}  // namespace

void cert_free(ttup_wasb* net) {
    CertState& c = net->cert;
    if (c.cropnet) { ttup_wasb_destroy(c.cropnet); c.cropnet = nullptr; }
    for (auto& sl : c.slot) {
        if (sl.mem) (void)hipFree(sl.mem);
        for (hipEvent_t e : {sl.done, sl.read_status, sl.read_info, sl.read_margin}) if (e) (void)hipEventDestroy(e);
        sl = CertState::Slot();
    }
    if (c.stats) (void)hipFree(c.stats);
    if (c.crop_heat) (void)hipFree(c.crop_heat);
    if (c.stream) (void)hipStreamDestroy(c.stream);
    if (c.lanes_done) (void)hipEventDestroy(c.lanes_done);
    c.stats = nullptr; c.crop_heat = nullptr; c.stream = nullptr; c.lanes_done = nullptr;
    c.enabled = false;
}

int cert_begin(ttup_wasb* net, int /*batch*/, hipStream_t caller) {
    CertState& c = net->cert;
    c.cur ^= 1;
    CertState::Slot& sl = c.slot[c.cur];
    TTUP_HIP_CHECK(hipStreamWaitEvent(caller, sl.done, 0));          // the call that last used this slot has finished its fp32 passes
    TTUP_HIP_CHECK(hipStreamWaitEvent(caller, sl.read_status, 0));   // ... and its caller's status / info copies have been made
    TTUP_HIP_CHECK(hipStreamWaitEvent(caller, sl.read_info, 0));
    TTUP_HIP_CHECK(hipStreamWaitEvent(caller, sl.read_margin, 0));   // (own event: hipEventRecord overwrites, and the margin copy may be issued on another stream than the status copy)
    TTUP_HIP_CHECK(hipMemsetAsync(sl.cand_cnt, 0, slot_zeroed_bytes(net), caller));          // cand_cnt, guard_cnt, status, n_crops (carve_slot)
    return TTUP_OK;
}

int cert_scan(ttup_wasb* net, const float* heat, const long long* argmax, int b0, int mb, hipStream_t st) {
    CertState& c = net->cert;
    CertState::Slot& sl = c.slot[c.cur];
    const int C = net->n_out;          // heat: (mb, C, H, W) -- map index = frame * C + channel
    const size_t m0 = (size_t)b0 * C;
    if (int rc = launch_scan(heat, argmax, mb * C, (long long)net->H * net->W, 2.f * c.eps, c.K, sl.cand_idx + m0 * c.K, sl.cand_cnt + m0,
                             sl.cand_bf + m0 * c.K, 2.f * c.eps * CertState::GUARD, sl.guard_cnt + m0, st)) return rc;
    PlanArgs a;
    a.cand_idx = sl.cand_idx; a.cand_cnt = sl.cand_cnt; a.cand_crop = sl.cand_crop; a.crop_rec = sl.crop_rec; a.n_crops = sl.n_crops;
    a.status = sl.status; a.stats = c.stats; a.cand_bf = sl.cand_bf; a.K = c.K; a.maxc = c.maxc; a.max_crops = c.budget;
    a.H = net->H; a.W = net->W; a.Hc = c.Hc; a.Wc = c.Wc; a.R = c.R; a.frame0 = b0; a.C = C; a.maxf = c.maxf; a.exact = c.exact_windows ? 1 : 0; a.guard_cnt = sl.guard_cnt; a.margin = sl.margin;
    a.audit_mod = c.audit_mod; a.audit_phase = c.audit_phase;
    a.small = c.small;
    hipLaunchKernelGGL(cert_plan_kernel, dim3(mb), dim3(64), 0, st, a);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

int cert_finish(ttup_wasb* net, const float* x_dev, const uint8_t* frames_dev, int n_frames, int src_h, int src_w, int batch,
                int64_t* argmax_dev, float* win_dev, hipStream_t caller) {
    CertState& c = net->cert;
    CertState::Slot& sl = c.slot[c.cur];
    ttup_wasb* cn = c.cropnet;
    // the fp32 passes run on the handle's own stream, behind everything the caller's stream has seen (the bf16 micro-batches
    // have been joined into it): a following call issued on ANOTHER caller stream overlaps with them
    hipStream_t st = c.stream;
    TTUP_HIP_CHECK(hipEventRecord(c.lanes_done, caller));
    TTUP_HIP_CHECK(hipStreamWaitEvent(st, c.lanes_done, 0));
    hipLaunchKernelGGL(cert_active_kernel, dim3(1), dim3(64), 0, st, sl.n_crops, sl.n_active, c.CH, c.nchunks, c.budget, (const CropRec*)sl.crop_rec, sl.roi_flag,
                       net->H, net->W, c.Hc, c.Wc);
    TTUP_LAUNCH_CHECK();
    // fp32 passes that can hold crops of THIS call: at most maxc per heatmap, at most the caller's budget
    const int C = net->n_out;
    int nch = cdiv(batch * c.maxf < c.budget ? batch * c.maxf : c.budget, c.CH);
    nch = nch > c.nchunks ? c.nchunks : nch;
    for (int ch = 0; ch < nch; ++ch) {
        const int crop0 = ch * c.CH;
        const int* na = sl.n_active + ch;
        cn->use_lane(0);
        float* xin = (float*)cn->tensors[cn->t_input].ptr;
        if (frames_dev) {
            const int rc = launch_preprocess_crops(frames_dev, n_frames, src_h, src_w, net->H, net->W, xin, sl.crop_rec, crop0, na, c.CH, c.Hc, c.Wc, net->in_ch / 3, st);
            if (rc) return rc;
        } else {
            const long long total = (long long)c.CH * c.Hc * c.Wc;
            hipLaunchKernelGGL(cert_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x_dev, net->in_ch, net->H, net->W,
                               (const CropRec*)sl.crop_rec, crop0, na, c.Hc, c.Wc, xin, total);
            TTUP_LAUNCH_CHECK();
        }
        cn->n_active = na;
        cn->roi_flag = cn->op_roi.empty() ? nullptr : sl.roi_flag + crop0;
        Roi hr = cn->out_roi; hr.flag = cn->roi_flag;
        int rc = run_ops(cn, c.CH, st);
        if (rc == TTUP_OK) rc = launch_head(cn->tensors[cn->t_out].ptr, cn->head_w_dev, cn->head_b_dev, C, c.crop_heat, c.CH, c.Hc, c.Wc, 16, TTUP_DTYPE_F32, st, na, &hr);
        cn->n_active = nullptr; cn->roi_flag = nullptr;
        if (rc) return rc;
        const int nthr = batch * C * c.K;
        hipLaunchKernelGGL(cert_lookup_kernel, dim3(cdiv(nthr, 256)), dim3(256), 0, st, (const int*)sl.cand_idx, (const int*)sl.cand_cnt, (const int*)sl.cand_crop,
                           (const int*)sl.status, (const CropRec*)sl.crop_rec, (const float*)c.crop_heat, c.K, net->H, net->W, c.Hc, c.Wc, crop0, c.CH, batch * C,
                           sl.cand_val, sl.cand_win, (const float*)sl.cand_bf, c.stats, C);
        TTUP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(cert_resolve_kernel, dim3(cdiv(batch * C, 64)), dim3(64), 0, st, (const int*)sl.cand_idx, (const int*)sl.cand_cnt, sl.status,
                       (const float*)sl.cand_val, (const float*)sl.cand_win, c.K, batch * C, (long long*)argmax_dev, win_dev, sl.margin);
    TTUP_LAUNCH_CHECK();
    TTUP_HIP_CHECK(hipEventRecord(sl.done, st));
    TTUP_HIP_CHECK(hipStreamWaitEvent(caller, sl.done, 0));          // outputs are final in the caller's stream order
    return TTUP_OK;
}

}  // namespace ttup

using namespace ttup;

int ttup_wasb_create_internal(const void* blob, size_t blob_bytes, int height, int width, int max_batch, int dtype, int micro, int lanes, ttup_wasb** out);

extern "C" int ttup_wasb_set_certify(ttup_wasb* net, float eps_abs, int crop, int max_crops_per_map) {
    TTUP_REQUIRE(net, TTUP_EINVAL, "ttup_wasb_set_certify: null handle");
    if (eps_abs < 0.f) { (void)hipDeviceSynchronize(); cert_free(net); return TTUP_OK; }
    TTUP_REQUIRE(net->dtype == TTUP_DTYPE_BF16, TTUP_EINVAL,
                 "ttup_wasb_set_certify: the certified argmax applies to bf16 handles (an fp32 handle's argmax is the fp32 argmax)");
    TTUP_REQUIRE(eps_abs == eps_abs && cert_args_ok(crop, max_crops_per_map), TTUP_EINVAL, "ttup_wasb_set_certify: bad argument");
    CertState& c = net->cert;
    if (c.enabled) { c.eps = eps_abs; if (crop == 0 && max_crops_per_map == 0) return TTUP_OK; }
    (void)hipDeviceSynchronize();
    cert_free(net);
    c.eps = eps_abs;
    c.small = 0;
    TTUP_REQUIRE(c.K <= CERT_MAX_K, TTUP_EINVAL, "ttup_wasb_set_certify: candidate list %d longer than the plan kernel's %d", c.K, CERT_MAX_K);
    const CertSizing s = cert_sizing(net->H, net->W, net->max_batch, net->n_out, crop, max_crops_per_map, cert_knobs());
    TTUP_REQUIRE(s.rc == TTUP_OK, s.rc, "%s", s.msg);
    c.maxc = s.maxc; c.maxf = s.maxf; c.Hc = s.Hc; c.Wc = s.Wc; c.CH = s.CH; c.max_crops = s.max_crops; c.nchunks = s.nchunks; c.budget = s.budget;
    const size_t nb = (size_t)net->max_batch * net->n_out;          // heatmaps per call
    for (auto& sl : c.slot) {
        TTUP_HIP_CHECK(hipMalloc(&sl.mem, carve_slot(sl, 0, nb, c.K, c.max_crops, c.nchunks)));
        carve_slot(sl, (uintptr_t)sl.mem, nb, c.K, c.max_crops, c.nchunks);
        TTUP_HIP_CHECK(hipMemsetD32((hipDeviceptr_t)sl.margin, 0x7f800000, nb));          // +inf: heatmaps never planned or resolved (ttup.h)
        TTUP_HIP_CHECK(hipMemset(sl.status, 0, nb * sizeof(int)));
        for (hipEvent_t* e : {&sl.done, &sl.read_status, &sl.read_info, &sl.read_margin}) TTUP_HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    TTUP_HIP_CHECK(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    TTUP_HIP_CHECK(hipEventCreateWithFlags(&c.lanes_done, hipEventDisableTiming));
    TTUP_HIP_CHECK(hipMalloc((void**)&c.stats, CERT_N_STATS * sizeof(unsigned long long)));
    TTUP_HIP_CHECK(hipMemset(c.stats, 0, CERT_N_STATS * sizeof(unsigned long long)));
    TTUP_HIP_CHECK(hipMalloc((void**)&c.crop_heat, (size_t)c.CH * net->n_out * c.Hc * c.Wc * sizeof(float)));
    const int rc = ttup_wasb_create_internal(net->blob.data(), net->blob.size(), c.Hc, c.Wc, c.CH, TTUP_DTYPE_F32, c.CH, 1, &c.cropnet);
    if (rc) { cert_free(net); return rc; }
    if (s.cone) {          // the crop net produces only what the core's rows / columns [R, side - R) depend on (class 2: [R, R + small + 2))
        c.small = s.small;
        const int rc2 = compute_roi(c.cropnet, c.R, c.Hc - c.R, c.R, c.small ? c.R + c.small + 2 : c.R);
        if (rc2) { cert_free(net); return rc2; }
    }
    c.enabled = true;
    return TTUP_OK;
}

extern "C" int ttup_wasb_certify_budget(ttup_wasb* net, int max_crops) {
    TTUP_REQUIRE(net && net->cert.enabled, TTUP_EINVAL, "ttup_wasb_certify_budget: the certified argmax is not enabled on this handle");
    TTUP_REQUIRE(max_crops >= 1, TTUP_EINVAL, "ttup_wasb_certify_budget: budget must be positive");
    net->cert.budget = max_crops < net->cert.max_crops ? max_crops : net->cert.max_crops;
    return TTUP_OK;
}

// The scan on its own (measurement aid and test hook): candidates of n_maps fp32 heatmaps within 2*eps_abs of each map's value at
// argmax_dev[map].  cand_cnt_dev must be zeroed by the caller; cand_idx_dev / cand_bf_dev hold K entries per map.
extern "C" int ttup_certify_scan(const float* heat_dev, const int64_t* argmax_dev, int n_maps, int height, int width, float eps_abs, int K,
                                 int* cand_idx_dev, int* cand_cnt_dev, float* cand_bf_dev, void* stream) {
    TTUP_REQUIRE(heat_dev && argmax_dev && cand_idx_dev && cand_cnt_dev && cand_bf_dev, TTUP_EINVAL, "ttup_certify_scan: null pointer");
    TTUP_REQUIRE(n_maps >= 0 && height > 0 && width > 0 && ((long long)height * width) % 4 == 0 && K > 0 && eps_abs >= 0.f, TTUP_EINVAL, "ttup_certify_scan: bad argument");
    if (n_maps == 0) return TTUP_OK;
    return launch_scan(heat_dev, (const long long*)argmax_dev, n_maps, (long long)height * width, 2.f * eps_abs, K, cand_idx_dev, cand_cnt_dev, cand_bf_dev,
                       0.f, nullptr, (hipStream_t)stream);
}

extern "C" int ttup_wasb_certify_exact_windows(ttup_wasb* net, int on) {
    TTUP_REQUIRE(net && net->cert.enabled, TTUP_EINVAL, "ttup_wasb_certify_exact_windows: the certified argmax is not enabled on this handle");
    net->cert.exact_windows = on != 0;
    return TTUP_OK;
}

extern "C" int ttup_wasb_certify_audit_crops(ttup_wasb* net, int every, int phase) {
    TTUP_REQUIRE(net && net->cert.enabled, TTUP_EINVAL, "ttup_wasb_certify_audit_crops: the certified argmax is not enabled on this handle");
    TTUP_REQUIRE(every >= 0 && phase >= 0, TTUP_EINVAL, "ttup_wasb_certify_audit_crops: every and phase must not be negative");
    net->cert.audit_mod = every;
    net->cert.audit_phase = every > 0 ? phase % every : 0;
    return TTUP_OK;
}

namespace ttup { namespace {
__global__ void cert_status_copy_kernel(const int* __restrict__ src, int* __restrict__ dst, int n, int mask) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i] & mask;
}
// the checks of the per-heatmap getters: `batch` values of the handle's last forward go to `out`
int check_getter(ttup_wasb* net, const void* out, int batch, const char* who) {
    TTUP_REQUIRE(net && out, TTUP_EINVAL, "%s: null pointer", who);
    TTUP_REQUIRE(net->cert.enabled, TTUP_EINVAL, "%s: the certified argmax is not enabled on this handle", who);
    TTUP_REQUIRE(batch >= 0 && batch <= net->max_batch * net->n_out, TTUP_EINVAL, "%s: %d heatmaps outside [0,%d]", who, batch, net->max_batch * net->n_out);
    return TTUP_OK;
}
int copy_status(ttup_wasb* net, int batch, int* status_dev, int mask, hipStream_t st, const char* who) {
    if (int rc = check_getter(net, status_dev, batch, who)) return rc;
    CertState::Slot& sl = net->cert.slot[net->cert.cur];
    if (batch > 0) {
        hipLaunchKernelGGL(cert_status_copy_kernel, dim3(cdiv(batch, 256)), dim3(256), 0, st, (const int*)sl.status, status_dev, batch, mask);
        TTUP_LAUNCH_CHECK();
    }
    TTUP_HIP_CHECK(hipEventRecord(sl.read_status, st));
    return TTUP_OK;
}
} }

extern "C" int ttup_wasb_certify_info(ttup_wasb* net, int* info_dev, void* stream) {
    if (int rc = check_getter(net, info_dev, 0, "ttup_wasb_certify_info")) return rc;
    CertState::Slot& sl = net->cert.slot[net->cert.cur];
    TTUP_HIP_CHECK(hipMemcpyAsync(info_dev, sl.n_crops, sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    TTUP_HIP_CHECK(hipMemcpyAsync(info_dev + 1, net->cert.stats + CS_max_candidate_err, sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));      // low word (little endian)
    TTUP_HIP_CHECK(hipEventRecord(sl.read_info, (hipStream_t)stream));
    return TTUP_OK;
}


// 0 / 1 / 2 per heatmap, as in ABI version 100 (the guard bit is NOT part of this value: callers compare it with 1 and 2)
extern "C" int ttup_wasb_certify_status(ttup_wasb* net, int batch, int* status_dev, void* stream) {
    return copy_status(net, batch, status_dev, CERT_STATUS_MASK, (hipStream_t)stream, "ttup_wasb_certify_status");
}
// fp32 top-2 margin among the candidates of every heatmap of the last forward (+inf for single-candidate / unresolved heatmaps)
extern "C" int ttup_wasb_certify_margins(ttup_wasb* net, int batch, float* margin_dev, void* stream) {
    if (int rc = check_getter(net, margin_dev, batch, "ttup_wasb_certify_margins")) return rc;
    CertState::Slot& sl = net->cert.slot[net->cert.cur];
    if (batch > 0) TTUP_HIP_CHECK(hipMemcpyAsync(margin_dev, sl.margin, (size_t)batch * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    TTUP_HIP_CHECK(hipEventRecord(sl.read_margin, (hipStream_t)stream));
    return TTUP_OK;
}
// status | CERT_GUARD where the guard band is not empty
extern "C" int ttup_wasb_certify_flags(ttup_wasb* net, int batch, int* flags_dev, void* stream) {
    return copy_status(net, batch, flags_dev, CERT_FLAGS_MASK, (hipStream_t)stream, "ttup_wasb_certify_flags");
}

extern "C" int ttup_wasb_certify_stats(ttup_wasb* net, long long* out_host, int reset) {
    if (int rc = check_getter(net, out_host, 0, "ttup_wasb_certify_stats")) return rc;
    TTUP_HIP_CHECK(hipDeviceSynchronize());
    TTUP_HIP_CHECK(hipMemcpy(out_host, net->cert.stats, CERT_N_STATS * sizeof(long long), hipMemcpyDeviceToHost));
    if (reset) TTUP_HIP_CHECK(hipMemset(net->cert.stats, 0, CERT_N_STATS * sizeof(long long)));
    return TTUP_OK;
}
