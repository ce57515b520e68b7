/*
 * ttup.h -- C ABI of libttup.so: the MI355X (gfx950) implementation of the
 * detect -> refine -> uplift hot path of KieDani/UpliftingTableTennis.
 *
 * The reference has no native code on this path: its boundary is three Python call sites
 * (SURVEY.md 8b).  Each entry point below names the reference call it replaces; the ctypes
 * binding a maintainer would add on the reference side is shown in INTEGRATION.md and is what
 * upliftingtabletennis_amd/_lib.py contains.
 *
 * Conventions
 *   - every pointer marked "dev" is device memory on the current HIP device, owned by the caller
 *     (torch tensors: tensor.data_ptr()), alive until `stream` has been synchronised;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream), 0 = default;
 *   - all functions return 0 on success, a TTUP_E* code otherwise; ttup_last_error() returns the
 *     thread-local message of the last failure;
 *   - handles own only their packed weights and scratch; create/destroy synchronise, forward never does;
 *   - no entry point falls back to the CPU: without a usable HIP device every compute call fails.
 */
#ifndef TTUP_H
#define TTUP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTUP_OK          0
#define TTUP_EINVAL      1   /* bad argument (Python shim raises ValueError)            */
#define TTUP_EFORMAT     2   /* weight blob does not match the architecture             */
#define TTUP_EHIP        3   /* HIP runtime error (RuntimeError)                        */
#define TTUP_ENOMEM      4
#define TTUP_EMASK       5   /* uplift mask is not {0,1} with at least one 0: the reference's
                                ValueError at uplifting/model.py:541-546                */
#define TTUP_ESTALE      6   /* the handle's weights were trained (ttup_uplift_opt_step): its packed
                                forward weights are stale, build an inference model from the trainer */

/* activation / arithmetic type of the CNN */
#define TTUP_DTYPE_BF16  0   /* bf16 storage, bf16 MFMA, fp32 accumulate (production)   */
#define TTUP_DTYPE_F32   1   /* fp32 storage and arithmetic (parity / debug path)       */

/* refine variants */
#define TTUP_REFINE_BALL  0  /* balldetection/helper_balldetection.py:29-110            */
#define TTUP_REFINE_TABLE 1  /* tabledetection/helper_tabledetection.py:50-156          */

/* channel order flag of ttup_preprocess */
#define TTUP_LAYOUT_NCHW_F32 0
#define TTUP_LAYOUT_NHWC16   1

typedef struct ttup_wasb   ttup_wasb;
typedef struct ttup_uplift ttup_uplift;
typedef struct ttup_vitpose ttup_vitpose;
typedef struct ttup_uplift_opt ttup_uplift_opt;

int         ttup_version(void);
/* 16 hex digits: the hash of the sources (every .hip and .h under csrc/, include/ttup.h) and compiler flags this library was built
 * from, compiled in by upliftingtabletennis_amd/build.py (source_id()).  The Python binding refuses a library whose id differs
 * from its source tree's, so a run proves which kernels it ran. */
const char* ttup_build_id(void);
const char* ttup_last_error(void);
/* number of visible HIP devices, <0 on error; does not initialise a context */
int         ttup_device_count(void);

/* ---------------------------------------------------------------- a1: pre-processing
 * Replaces balldetection/transforms.py:17-52 (cv2.resize, INTER_LINEAR, uint8), :379-402
 * (x/255, ImageNet mean/std) and the triple concat of interface.py:104-112.
 * frames_dev: (n_frames, src_h, src_w, 3) uint8, channel order as delivered (BGR on the hub surface).
 * Triple t uses frames t, t+1, t+2 -> n_triples = n_frames-2 outputs.
 * out_dev: float32 (n_triples, 9, dst_h, dst_w) NCHW -- the tensor interface.py:112 feeds the model.
 */
int ttup_preprocess_triples(const uint8_t* frames_dev, int n_frames, int src_h, int src_w,
                            int dst_h, int dst_w, float* out_dev, void* stream);

/* single frames (table detector, tabledetection/transforms.py:17-38 + NormalizeImage; interface.py:160-165):
 * frames_dev (n,src_h,src_w,3) uint8 -> out_dev float32 (n,3,dst_h,dst_w) */
int ttup_preprocess_frames(const uint8_t* frames_dev, int n_frames, int src_h, int src_w,
                           int dst_h, int dst_w, float* out_dev, void* stream);

/* ---------------------------------------------------------------- a2: WASB / HRNet CNN
 * Replaces WASBNet.forward (balldetection/models/wasb.py:596-608) behind `self.model(x)`
 * (interface.py:115, inference/utils.py:57).
 *
 * blob: weights serialised by upliftingtabletennis_amd.weights.pack_wasb_blob:
 *   char magic[8]="TTUPWSB1"; int32 n_convs, in_ch, head_out, 0;
 *   per conv (order = reference state_dict order): int32 cout,cin,k,stride,has_bn,has_bias,0,0;
 *   float w[cout][cin][k][k]; if has_bias float b[cout]; if has_bn float gamma,beta,mean,var [cout] each.
 * BN folding (eps 1e-5) and MFMA fragment packing happen inside create.
 * height/width: network input size (multiples of 8); max_batch: largest B accepted by forward.
 * The same entry points serve the table-keypoint HRNet (tabledetection/models/hrnet.py:510-589): a blob with
 * in_ch=3, head_out=13 gives a handle whose forward takes (B,3,H,W) and returns all 13 heatmap channels (B,13,H,W);
 * argmax/win outputs then hold B*13 entries.  head_out=3 (ball) returns only channel 1, as WASBNet.forward does.
 */
int  ttup_wasb_create(const void* blob, size_t blob_bytes, int height, int width, int max_batch,
                      int dtype, ttup_wasb** out);
/* The same with the batching fixed by the caller: forward splits a batch into micro-batches of `micro_batch` samples and runs them
 * round-robin on `lanes` internal streams (0 = the defaults: 8 and 2).  lanes = 1: everything on the caller's stream -- for a
 * handle that runs side by side with another busy handle (the hub pipeline's table and ball detectors). */
int  ttup_wasb_create_ex(const void* blob, size_t blob_bytes, int height, int width, int max_batch,
                         int dtype, int micro_batch, int lanes, ttup_wasb** out);
void ttup_wasb_destroy(ttup_wasb* net);
/* The handle's internal HIP streams -> out[0..*n_out): the lane streams (none for a single-lane handle), then the stream of the
 * certified argmax's fp32 passes when it is enabled.  HIP maps all streams of a process onto a few hardware queues; work on two
 * streams of one queue never overlaps (tools/queue_probe.py measures which ones do). */
int  ttup_wasb_streams(ttup_wasb* net, void** out, int cap, int* n_out);

/* x_dev: float32 (B,9,H,W) NCHW.  heat_dev: float32 (B,1,H,W) (nullable).
 * argmax_dev: int64 (B) flat index of the first maximum of each heatmap (nullable).
 * win_dev: float32 (B,9) zero-padded 3x3 window around it (nullable). */
int ttup_wasb_forward(ttup_wasb* net, const float* x_dev, int batch, float* heat_dev,
                      int64_t* argmax_dev, float* win_dev, void* stream);

/* Fused fast path: uint8 frames in, heatmaps / peaks out (pre-processing runs inside).
 * frames_dev: (n_frames, src_h, src_w, 3) uint8; produces n_frames-2 heatmaps (triples t,t+1,t+2). */
int ttup_wasb_forward_frames(ttup_wasb* net, const uint8_t* frames_dev, int n_frames, int src_h, int src_w,
                             float* heat_dev, int64_t* argmax_dev, float* win_dev, void* stream);

/* debug/test: copy an internal activation ("stem1","stem2","layer1","trans1_0","trans1_1","stage2_0",...,
 * "stage4_0") of the last forward as float32 NCHW into out_dev; *c,*h,*w receive its shape. */
int ttup_wasb_read_tap(ttup_wasb* net, const char* name, int batch, float* out_dev, int* c, int* h, int* w, void* stream);

/* measurement aids (bench.py), HIP events on `stream`; see csrc/wasb_net.hip.  time_ops: every op on its own (warm inputs);
 * time_graph: the whole graph in launch order with an event between consecutive ops (the cache state the forward pass sees),
 * names_out = max_ops x 64 chars receiving the HIP kernel name of each op (nullable). */
int ttup_wasb_time_ops(ttup_wasb* net, int batch, int reps, int max_ops, float* ms_out, int* info_out, int* n_ops_out, void* stream);
int ttup_wasb_time_graph(ttup_wasb* net, int batch, int reps, int max_ops, float* ms_out, int* info_out, char* names_out,
                         int* n_ops_out, void* stream);
/* time_replay: the same launches back to back, `reps` passes between one pair of events (none between the ops); ms_out[0] = average
 * duration of a pass of the graph over one micro-batch (ABI 103). */
int ttup_wasb_time_replay(ttup_wasb* net, int batch, int reps, float* ms_out, void* stream);
/* measured peaks of the device (csrc/peaks.hip; SURVEY 8d "Peaks to divide by"), HIP events on `stream`, synchronises.
 * mfma: out_host[0..1] = TFLOP/s of register-resident v_mfma_f32_16x16x32_bf16 / v_mfma_f32_32x32x16_bf16 loops on random
 * operands with `waves_per_simd` waves on every SIMD, [2..3] their durations (ms).
 * hbm: out_host[0..2] = GB/s of a streaming read / copy / triad over arrays of `bytes` each (>= 1 GiB: past the Infinity Cache),
 * [3..5] their durations (ms). */
int ttup_peak_mfma_bf16(int iters, int waves_per_simd, double* out_host, void* stream);
int ttup_peak_hbm(size_t bytes, double* out_host, void* stream);
/* Certified argmax for the bf16 ball detector (north_star: bit-exact heatmap argmax indices; reference
 * balldetection/helper_balldetection.py:50 takes torch.argmax of the fp32 heatmap).  eps_abs bounds |bf16 heatmap - fp32 heatmap|
 * (calibrated by the caller on its own frames; upliftingtabletennis_amd.wasb.WASBNet.calibrate).  Once set, every forward that
 * returns peaks re-evaluates the pixels within 2*eps_abs of the bf16 maximum on fp32 receptive-field crops (crop x crop pixels,
 * 0 = 168 = the 72-pixel receptive-field radius on both sides of a 24-pixel core; a multiple of 8, at least 160 (ABI 103); at most max_crops_per_map per heatmap, 0 = 8) inside the same call, without host synchronisation, and returns the
 * fp32 winner and its fp32 3x3 window.  eps_abs < 0 switches it off.  csrc/certify.hip.
 * status (after a forward, per heatmap; ttup_wasb_certify_status): 0 = one candidate (the bf16 index is certain), 1 = resolved on
 * fp32 crops, 2 = not certified (candidate / crop budget exceeded; the bf16 index is returned).
 * flags (ttup_wasb_certify_flags): the status with bit 2 (value 4) set when the GUARD band -- the pixels between 2*eps_abs and
 * 2*1.25*eps_abs below the maximum -- is not empty: a heatmap WITHOUT that bit has the same candidates, and so the same certified
 * result, under any eps up to 1.25*eps_abs (a caller that widens eps re-runs only the heatmaps with it).
 * Both copies (and ttup_wasb_certify_info) belong to the handle's LAST forward and are ordered by the library against the next
 * forward that reuses the per-call slot, whatever stream that one is issued on.
 * stats (cumulated, synchronises): {heatmaps, single-candidate, resolved, not certified, crops, candidates of resolved,
 * bits of max |bf16 - fp32| seen at a candidate (a float in the low 32 bits: the free part of the eps audit), single-candidate
 * heatmaps cropped in exact-window mode}. */
int ttup_wasb_set_certify(ttup_wasb* net, float eps_abs, int crop, int max_crops_per_map);
/* step 1 of the certification on its own (the kernel that streams the heatmap on the production path: measurement aid, test
 * hook): for each of n_maps fp32 heatmaps (n_maps, H, W) the pixels whose value is >= heat[argmax[map]] - 2*eps_abs, appended in
 * arbitrary order to cand_idx_dev[map*K ..] (flat pixel index) / cand_bf_dev (their values); cand_cnt_dev[map] (zeroed by the
 * caller) counts ALL of them, also those past K. */
int ttup_certify_scan(const float* heat_dev, const int64_t* argmax_dev, int n_maps, int height, int width, float eps_abs, int K,
                      int* cand_idx_dev, int* cand_cnt_dev, float* cand_bf_dev, void* stream);
/* max |a - b| over n floats -> out_dev[0] (device, written on `stream`; NaN anywhere gives NaN).  The eps audit's error measure
 * (upliftingtabletennis_amd/wasb.py: heatmap_error): one pass over the two heatmaps instead of three torch kernels, and free of
 * packed fp32 instructions, which must not run beside the CNN (csrc/common.h). */
int ttup_max_abs_diff(const float* a_dev, const float* b_dev, long long n, float* out_dev, void* stream);
/* the same over the columns [c0, c1) of `rows` rows of `width` floats (a strip audit leaves out the columns whose receptive field
 * reaches the strip's artificial border); accumulate != 0 keeps the running maximum already in out_dev[0] */
int ttup_max_abs_diff_cols(const float* a_dev, const float* b_dev, long long rows, long long width, long long c0, long long c1,
                           float* out_dev, int accumulate, void* stream);
/* dst[r][j] = src[r][x0 + j] for r < rows, j < w: a column strip of a (rows, width) float array (the audit's strip of the
 * pre-processed input, without torch's copy kernels on the audit stream) */
int ttup_slice_columns(const float* src_dev, long long rows, int width, int x0, int w, float* dst_dev, void* stream);
/* exact-window mode (on != 0): heatmaps with ONE candidate get an fp32 crop too, so that every returned 3x3 window -- not only
 * the near-ties' -- holds the fp32 path's values and the sub-pixel fit sees what the reference's fit sees (one 168x168 fp32
 * pass per heatmap: a parity / audit mode, off by default) */
int ttup_wasb_certify_exact_windows(ttup_wasb* net, int on);
/* audit crops (every > 0): of the frames f of the following forwards with (f + phase) % every == 0, ONE single-candidate heatmap
 * (channel (f / every) % channels) gets an fp32 crop although its index is already certain; like every crop it reports
 * |bf16 - fp32| at its candidate into the running maximum that ttup_wasb_certify_info returns.  This is the candidate-level audit
 * extended to heatmaps WITHOUT near-ties (reference: helper_balldetection.py:50 takes the argmax of an fp32 heatmap; the bound on
 * |bf16 - fp32| is what lets the bf16 path return the same index).  every = 0 switches it off (default). */
int ttup_wasb_certify_audit_crops(ttup_wasb* net, int every, int phase);
/* info_dev[0] = crops the LAST forward asked for (may exceed the budget it had); info_dev[1] = the bits of a float: the largest
 * |bf16 - fp32| seen so far at any candidate of any call (stats[6]); both copied in stream order, no synchronisation */
int ttup_wasb_certify_info(ttup_wasb* net, int* info_dev, void* stream);
int ttup_wasb_certify_status(ttup_wasb* net, int batch, int* status_dev, void* stream);
int ttup_wasb_certify_flags(ttup_wasb* net, int batch, int* flags_dev, void* stream);
/* measurement: by how much the fp32 winner of each heatmap of the last forward leads the best OTHER candidate on the fp32 crops
 * (float32 (batch); +inf where there was one candidate or the heatmap was not resolved).  A margin below the accuracy of the fp32
 * path against the reference's own fp32 arithmetic marks a heatmap whose argmax the reference itself does not determine. */
int ttup_wasb_certify_margins(ttup_wasb* net, int batch, float* margin_dev, void* stream);
/* crops the following forward calls may use (default: max_batch, i.e. one per sample): the call enqueues ceil(budget / CH) fp32
 * passes sized on the device (CH = min(max_batch, 128) crops per pass; 64 before ABI 103; TTUP_CERT_CH), so a caller that knows its
 * typical crop count (stats / status of earlier calls) saves the empty passes; heatmaps beyond the budget are flagged 2 */
int ttup_wasb_certify_budget(ttup_wasb* net, int max_crops);
/* running counters of the handle since creation / the last reset, copied to TWELVE long longs on the host (synchronises): [0] heatmaps,
 * [1] single candidate (status 0, audit picks included), [2] resolved on fp32 crops (status 1), [3] not certified (status 2, = [8] + [9]
 * + [10]; [1] + [2] + [3] = [0]), [4] crops, [5] candidates of the resolved heatmaps, [6] low word = bits of the largest |bf16 - fp32|
 * seen at a candidate, [7] single-candidate heatmaps whose crop was kept (exact-window mode / audit crops; one dropped for lack of
 * room is not counted), [8] not certified: candidate list overflow, [9]: more crops than one heatmap / frame may add,
 * [10]: the call's crop list was full, [11] crops of class 2 among [4] (candidates within a 14-position core: pruned to a smaller cone;
 * ABI 103).  (ABI version 100 copied eight.) */
int ttup_wasb_certify_stats(ttup_wasb* net, long long* out_host12, int reset);
/* scheduling priority of the handle's internal streams (high != 0: greatest device priority); synchronises */
int ttup_wasb_set_priority(ttup_wasb* net, int high);
/* micro-batch the handle was created with (TTUP_MICRO_BATCH) */
int ttup_wasb_micro_batch(ttup_wasb* net);
/* heatmap channels per sample returned by forward: 1 (ball) or 13 (table) */
int ttup_wasb_out_channels(ttup_wasb* net);

/* ---------------------------------------------------------------- a2': ViTPose-small detector (csrc/vitpose.hip)
 * Replaces VitPose.forward (balldetection/models/vitpose.py:92-103, classify_invisible=False; tabledetection/models/vitpose.py)
 * behind `self.model(x)` for model_name 'vitpose'.  ttup_vitpose_create: fp32 arithmetic throughout (fp32-operand MFMA).
 * ttup_vitpose_create_dtype with dtype 1: the bf16 path on the bf16 matrix pipe (bf16 matrix weights and stored activations, fp32
 * residual stream, softmax, accumulation and heatmap, fp64 LayerNorms: DESIGN.md section 24) -- an uncertified detector, meant for the
 * hub's aux slot; dtype 0 is ttup_vitpose_create.  forward / forward_frames dispatch on the handle.
 * blob: upliftingtabletennis_amd.weights.pack_vitpose_blob:
 *   char magic[8]="TTUPVIT1"; int32 in_ch, out_ch, 384, 12 (depth), 12 (heads), 1536 (mlp), 256 (deconv), n_pos;
 *   float pos_embed[n_pos][384]; patch w[384][in_ch][16][16], b[384];
 *   12 x { norm1 w,b[384]; qkv w[1152][384], b[1152]; proj w[384][384], b[384]; norm2 w,b[384]; fc1 w[1536][384], b[1536];
 *          fc2 w[384][1536], b[384] };  last_norm w,b[384];
 *   deconv 1: w[4][256][4*384], b[256]; deconv 2: w[4][256][4*256], b[256] -- each ConvTranspose2d(k4,s2,p1) + BN folded into four
 *   2x2 sub-convolutions (phase 2*py+px, reduction index (2*dy+dx)*cin + c; weights.vitpose_fold_head);  final w[out_ch][256], b[out_ch].
 * height/width: network input (multiples of 16; n_pos must be (height/16)*(width/16)+1); max_batch: largest B of forward;
 * micro_batch: samples per internal pass (0 = min(8, max_batch)); out_ch 1 (ball) or up to 16 (13: table keypoints). */
int  ttup_vitpose_create(const void* blob, size_t blob_bytes, int height, int width, int max_batch, int micro_batch,
                         int in_ch, int out_ch, ttup_vitpose** out);
int  ttup_vitpose_create_dtype(const void* blob, size_t blob_bytes, int height, int width, int max_batch, int micro_batch,
                               int in_ch, int out_ch, int dtype, ttup_vitpose** out);
void ttup_vitpose_destroy(ttup_vitpose* net);
int  ttup_vitpose_micro_batch(ttup_vitpose* net);
/* x_dev: float32 (B,in_ch,H,W) NCHW, 16-byte aligned.  heat_dev: float32 (B,out_ch,H/4,W/4) (nullable).
 * argmax_dev: int64 (B*out_ch) flat index of the first maximum of each heatmap, win_dev: float32 (B*out_ch,9) zero-padded 3x3
 * window around it (both or neither). */
int  ttup_vitpose_forward(ttup_vitpose* net, const float* x_dev, int batch, float* heat_dev, int64_t* argmax_dev,
                          float* win_dev, void* stream);
/* frames_dev: n_frames BGR uint8 (src_h,src_w,3) HWC frames on the device, any size.  Samples: n_frames - 2 triples (t, t+1, t+2)
 * for a 9-channel handle, n_frames frames for a 3-channel one (at most max_batch).  Outputs as ttup_vitpose_forward, bit-identical
 * to it on ttup_preprocess_triples / ttup_preprocess_frames of the same frames; each frame is pre-processed once. */
int  ttup_vitpose_forward_frames(ttup_vitpose* net, const uint8_t* frames_dev, int n_frames, int src_h, int src_w, float* heat_dev,
                                 int64_t* argmax_dev, float* win_dev, void* stream);
/* Testing seam: one stage alone on a given device input, batch <= micro_batch.  stage 0: the patch embedding of in_dev = x
 * (batch,in_ch,H,W); stages 1..12: block `stage` on in_dev = a float32 residual stream (batch*tokens,384); stage 13: the head
 * (last_norm, deconvolutions, final conv) on a residual stream.  ttup_vitpose_read_tap then copies what that stage left in the
 * handle's buffers to dst (host or device, exactly `bytes` long): stage 0 "x"; blocks "qkv", "att", "x_attn" (the residual stream
 * after the attention half), "hid", "x"; head "ln", "d1", "d2" (NHWC), "heat".  x, x_attn and heat are float32; the others are
 * float32 on an f32 handle and raw bf16 (uint16) on a bf16 handle.  An unknown tap, a tap the last stage did not write, a wrong
 * size, or a forward since the stage: TTUP_EINVAL. */
int  ttup_vitpose_run_stage(ttup_vitpose* net, int stage, const float* in_dev, int batch, void* stream);
int  ttup_vitpose_read_tap(ttup_vitpose* net, const char* tap, void* dst, size_t bytes);
/* The backbone alone: x_dev (batch,in_ch,H,W) float32 -> out_dev (batch*tokens,384) float32, last_norm's output (what the head's
 * deconvolutions read; bit-equal to the "ln" tap of stage 13 on the residual stream the blocks leave), in micro-batches, any batch >= 0.
 * An f32 handle only: a bf16 handle is TTUP_EINVAL. */
int  ttup_vitpose_features(ttup_vitpose* net, const float* x_dev, int batch, float* out_dev, void* stream);

/* ---------------------------------------------------------------- ViTPose head: training-mode forward and backward
 * The keypoint head (two ConvTranspose2d(k4,s2,p1,no bias) + BatchNorm2d(eps 1e-5, momentum 0.1) + ReLU, a 1x1 conv) with BN kept
 * apart from the weights, and its backward.  Parameters stay where the caller keeps them, in the reference's layouts (all device
 * pointers, float32; num_batches_tracked int64): the handle packs what its kernels read on every forward.  The handle owns one
 * workspace (ttup_vitpose_head_workspace_bytes) sized for max_rows tokens (batch * hp * wp) and out_ch in 1..16, and keeps the
 * activations of the last forward for the backward.
 * forward: feat_dev (batch*hp*wp, 384) token-major (sample, row, column), 16-byte aligned -> heat_dev (batch,out_ch,4hp,4wp).
 *   train != 0: BN takes the batch's mean and biased variance over (batch, H, W) and updates running_mean / running_var (the
 *   unbiased variance) / num_batches_tracked in place; train == 0: BN reads the running statistics and updates nothing.
 * backward: dheat_dev (batch,out_ch,4hp,4wp), the batch and grid of the last forward -> every gradient of ttup_vitpose_head_grads
 *   (overwritten, the reference's shapes; feat (batch*hp*wp, 384), 16-byte aligned), through BN in the mode the forward ran in.
 *   It may run more than once per forward.  Same inputs, same bits: no sum is atomic.
 * read_tap (testing seam): "z1", "a1" (batch,2hp,2wp,256) and "z2", "a2" (batch,4hp,4wp,256) NHWC, "mean1", "var1", "mean2", "var2"
 *   (256: the statistics the BN used) of the last forward, to dst (host or device, exactly `bytes` long).
 * TTUP_EINVAL before any device call: null pointers, out_ch outside 1..16, max_rows outside 1..2^22, a non-positive batch or grid,
 * more rows than max_rows, a backward without a forward or with another batch or grid than the forward's, an unknown tap or a
 * wrong size. */
typedef struct ttup_vitpose_head ttup_vitpose_head;
typedef struct ttup_vitpose_head_params {
    const float *deconv1_weight, *bn1_weight, *bn1_bias;          /* (384,256,4,4), (256), (256) */
    float *bn1_running_mean, *bn1_running_var;                    /* (256) each */
    int64_t* bn1_num_batches_tracked;                             /* (1) */
    const float *deconv2_weight, *bn2_weight, *bn2_bias;          /* (256,256,4,4), (256), (256) */
    float *bn2_running_mean, *bn2_running_var;
    int64_t* bn2_num_batches_tracked;
    const float *final_weight, *final_bias;                       /* (out_ch,256,1,1), (out_ch) */
} ttup_vitpose_head_params;
typedef struct ttup_vitpose_head_grads {
    float *deconv1_weight, *bn1_weight, *bn1_bias, *deconv2_weight, *bn2_weight, *bn2_bias, *final_weight, *final_bias, *feat;
} ttup_vitpose_head_grads;
size_t ttup_vitpose_head_workspace_bytes(int out_ch, long long max_rows);          /* 0: refused arguments */
int  ttup_vitpose_head_create(int out_ch, long long max_rows, ttup_vitpose_head** out);
void ttup_vitpose_head_destroy(ttup_vitpose_head* head);
int  ttup_vitpose_head_forward(ttup_vitpose_head* head, const float* feat_dev, int batch, int hp, int wp, const ttup_vitpose_head_params* params,
                               int train, float* heat_dev, void* stream);
int  ttup_vitpose_head_backward(ttup_vitpose_head* head, const float* dheat_dev, int batch, int hp, int wp, const ttup_vitpose_head_grads* grads,
                                void* stream);
int  ttup_vitpose_head_read_tap(ttup_vitpose_head* head, const char* tap, void* dst, size_t bytes);

/* ---------------------------------------------------------------- ViTPose backbone: training-mode forward and backward
 * The ViTPose-small backbone (Conv2d(k16,s16,p2) patch embedding + pos_embed, 12 pre-LN blocks, last_norm) with every block's
 * activations kept, and its backward.  The 149 tensors stay where the caller keeps them, in the reference's layouts (device
 * pointers, float32, 16-byte aligned), in the reference's state_dict order: pos_embed, patch_embed.proj.weight / .bias, per block
 * norm1.weight / .bias, attn.qkv.weight / .bias, attn.proj.weight / .bias, norm2.weight / .bias, mlp.fc1.weight / .bias,
 * mlp.fc2.weight / .bias, then last_norm.weight / .bias.  The handle owns one workspace (ttup_vitpose_grad_workspace_bytes) sized
 * for max_batch samples of hp x wp tokens and in_ch in 1..16.
 * forward: x_dev (batch,in_ch,16hp,16wp) -> feat_dev (batch*hp*wp, 384), last_norm's output.  drop_scale_dev: (12,2,batch) floats,
 *   the factor on residual branch (block, half) of every sample (stochastic depth: 0 or 1/keep), drop_scale_len its length; null
 *   and 0: every factor 1, and then feat is ttup_vitpose_features' bit for bit.
 * backward: dfeat_dev (batch*hp*wp, 384), the batch of the last forward and the same parameters -> the 149 gradients (overwritten,
 *   the parameters' shapes).  The gradient into the images is not computed.  It may run more than once per forward.  Same inputs,
 *   same bits: no sum is atomic.
 * read_tap (testing seam): "x" (block 0..12), "x_mid", "att" (rows,384), "qkv" (rows,1152), "lse" (rows,12), "pre" (rows,1536) of
 *   block 0..11 of the last forward, and "dqkv" (rows,1152; block 0) of the last backward, to dst (exactly `bytes` long).
 * TTUP_EINVAL before any device call: null pointers, in_ch outside 1..16, a non-positive grid or batch, more than 2^22 tokens, a
 *   batch beyond max_batch, a drop_scale of another length than 24 * batch, a backward without a forward or with another batch,
 *   an unknown tap or a wrong size. */
#define TTUP_VITPOSE_BACKBONE_TENSORS 149
typedef struct ttup_vitpose_grad ttup_vitpose_grad;
typedef struct ttup_vitpose_backbone_params { const float* t[TTUP_VITPOSE_BACKBONE_TENSORS]; } ttup_vitpose_backbone_params;
typedef struct ttup_vitpose_backbone_grads { float* t[TTUP_VITPOSE_BACKBONE_TENSORS]; } ttup_vitpose_backbone_grads;
size_t ttup_vitpose_grad_workspace_bytes(int in_ch, int hp, int wp, int max_batch);          /* 0: refused arguments */
int  ttup_vitpose_grad_create(int in_ch, int hp, int wp, int max_batch, ttup_vitpose_grad** out);
void ttup_vitpose_grad_destroy(ttup_vitpose_grad* h);
int  ttup_vitpose_grad_forward(ttup_vitpose_grad* h, const float* x_dev, int batch, const ttup_vitpose_backbone_params* params,
                               const float* drop_scale_dev, long long drop_scale_len, float* feat_dev, void* stream);
int  ttup_vitpose_grad_backward(ttup_vitpose_grad* h, const float* dfeat_dev, int batch, const ttup_vitpose_backbone_params* params,
                                const ttup_vitpose_backbone_grads* grads, void* stream);
int  ttup_vitpose_grad_read_tap(ttup_vitpose_grad* h, const char* tap, int block, void* dst, size_t bytes);

/* ---------------------------------------------------------------- a3/a4: heatmap argmax + refine
 * Replaces extract_position_torch_gaussian (ball: helper_balldetection.py:29-110, called at
 * inference/utils.py:59; table: helper_tabledetection.py:50-156, called at interface.py:116).
 * heat_dev: float32 (n_maps, H, W).  out_xyv_dev: float64 (n_maps,3) [x,y,visibility] in
 * img_w x img_h pixel coordinates.  argmax_dev / win_dev as above (nullable outputs).
 * ws_dev: scratch of at least ttup_refine_workspace_bytes(n_maps,H,W) bytes.
 */
size_t ttup_refine_workspace_bytes(int n_maps, int height, int width);
int ttup_refine(const float* heat_dev, int n_maps, int height, int width, int img_w, int img_h, int variant,
                double* out_xyv_dev, int64_t* argmax_dev, float* win_dev, void* ws_dev, size_t ws_bytes, void* stream);
/* second half only: peaks already known (from ttup_wasb_forward) */
int ttup_refine_windows(const int64_t* argmax_dev, const float* win_dev, int n_maps, int height, int width,
                        int img_w, int img_h, int variant, double* out_xyv_dev, void* stream);

/* ---------------------------------------------------------------- a6: uplift transformer
 * Replaces the forward of every model uplifting/model.py:574-603 get_model builds -- SingleStageModel (:393-499) and
 * MultiStageModel (:502-571) -- behind `self.model(ball, table, mask, times)` (interface.py:235, inference/utils.py:254).  The
 * variant travels in the blob; a blob with variant == 0 and time_rotation == 0 is 'connectstage' / 'dynamic' / 'new', the only
 * one earlier versions wrote.
 * blob: upliftingtabletennis_amd.weights.pack_uplift_blob:
 *   char magic[8]="TTUPUPL1";
 *   int32 dim, heads, n_pos_layers, n_first_layers, n_second_layers, n_table, variant, time_rotation;
 *     variant        = name | mode << 4; name: 0 connectstage, 1 multistage, 2 singlestage;
 *                      mode: 0 dynamic, 1 stacked, 2 originalmethod, 3 free (singlestage only; originalmethod not for singlestage)
 *     time_rotation  = 0 'new' (RoPE index round(t / 0.002 s)), 1 'old' (index of the token in its sequence)
 *     n_pos_layers   = 4 for mode dynamic, else 0; n_second_layers = 0 for singlestage (n_first_layers = depth), else 4
 *   then records, each int32 numel; float data[numel], weights row-major as in the state_dict:
 *     inv_freq (head_dim/2), cls_token (dim),
 *     ball_embed fc1.weight (dim x K), fc1.bias, fc2.weight, fc2.bias     K = 2; 41 stacked; 28 originalmethod
 *     table_embed fc1.weight (dim x 2), fc1.bias, fc2.weight, fc2.bias    mode dynamic only
 *     n_pos_layers + n_first_layers layers, each: qkv.weight, qkv.bias, proj.weight, mlp1.fc1.weight, .bias, mlp1.fc2.weight, .bias,
 *                                                 norm1.weight, .bias, norm2.weight, .bias
 *     position_head fc1.weight, .bias, fc2.weight, .bias, fc3.weight, .bias
 *     embed fc1.weight (dim x 3), fc1.bias, fc2.weight, fc2.bias          multistage only
 *     n_second_layers layers
 *     rotation_head (as position_head)
 *   This is state_dict order without the per-layer inv_freq, except that `embed` (present in both two-stage models' state dicts,
 *   read by multistage alone) moves in front of the second stage and singlestage's position head in front of its rotation head.
 * A 'connectstage' / 'dynamic' handle also keeps the records as plain fp32 on the device for ttup_uplift_loss_grad (one more copy of
 * the weights: 0.3 MB small, 1.7 MB base, 8.2 MB large, 18.5 MB huge), whether or not gradients are ever asked for.
 */
int  ttup_uplift_create(const void* blob, size_t blob_bytes, int max_batch, int max_len, ttup_uplift** out);
void ttup_uplift_destroy(ttup_uplift* net);
/* ball (B,T,2), table (B,13,3), mask (B,T) in {0,1}, times (B,T) seconds -> rot (B,3), pos (B,T,3); all float32 dev.
 * check_mask != 0 reproduces the reference's ValueError (TTUP_EMASK) and costs one stream synchronisation.
 * len is refused with TTUP_EINVAL, before anything is launched or captured, when it exceeds max_len or when the len + 1 tokens of the
 * cls stage exceed what the handle's attention kernels serve: 512 tokens for dim 128 / 4 heads (the matrix-pipe kernels), else the scalar
 * kernel's 64 KB of LDS -- 962 / 496 / 334 / 251 tokens for head dims 8 / 16 / 24 / 32 (the last one under TTUP_UPLIFT_SCALAR_ATTENTION
 * or TTUP_F32_EXACT).  ttup_uplift_create accepts a larger max_len; it sizes the scratch only. */
int ttup_uplift_forward(ttup_uplift* net, const float* ball_dev, const float* table_dev, const float* mask_dev,
                        const float* times_dev, int batch, int len, float* rot_dev, float* pos_dev,
                        int check_mask, void* stream);

/* Small batches (batch * len <= 1024 tokens) are replayed from a hipGraph captured on the second call with a given (batch, len).
 * out_host3[0] = graphs held, [1] = 1 when the graph path is off (capture failed on this runtime, or TTUP_UPLIFT_NO_GRAPH is set),
 * [2] = forwards served by a replay so far. */
int ttup_uplift_graph_info(ttup_uplift* net, int* out_host3);

/* Sequences of at most 64 tokens (the table stage always; the temporal and spin stages of clips of up to 63 frames) run ALL layers
 * of a stage in one launch with the tokens resident on the CU (TTUP_UPLIFT_NO_STAGE=1 switches it off, TTUP_UPLIFT_STAGE_WG caps the
 * launch size it is used for).  *out_host = such launches issued or captured so far. */
int ttup_uplift_stage_info(ttup_uplift* net, long long* out_host);

/* ---------------------------------------------------------------- uplift training loss and its parameter gradients (csrc/uplift_grad.hip)
 * Replaces, for one batch, the forward, the loss and `loss.backward()` of uplifting/train.py:121-128 for the configuration the
 * reference trains, get_model('connectstage', size, 'dynamic', time_rotation):
 *   loss_rot = sum_b ||pred_rot_b - rot_b||_2,  loss_pos = sum (pred_pos - r_world)^2 mask / sum mask,  loss = loss_rot + loss_pos.
 * A handle that holds any other variant is refused with TTUP_EINVAL before anything touches a device.  Clipping, the optimizer and
 * the EMA follow in ttup_uplift_opt_step (below).
 *
 * ttup_uplift_grad_layout: the flat gradient buffer holds the tensors of arch.uplift_variant_schema(name, size, mode) in that
 * order, without the `*.rotary_emb.inv_freq` buffers.  *n_floats = its length, *n_tensors = the number of tensors; offsets_host /
 * used_host (nullable, `capacity` entries each) receive every tensor's offset and whether it gets a gradient: the four `embed.*`
 * tensors, which 'connectstage' never reads (`.grad is None` in the reference), are present, written as zeros and marked 0.
 * ttup_uplift_grad_workspace_bytes: bytes of caller-allocated device scratch for a call with (batch, len); 0 for a null or
 * unsupported handle.  It grows with min(batch, 262144 / (14 len)) trajectories: larger batches are processed in groups of that size.
 * ttup_uplift_loss_grad: ball (B,T,2), table (B,13,3), mask (B,T) in {0,1}, times (B,T), r_world (B,T,3), rotation (B,3), all
 * float32 on the device.  flags bit 0: transform_mode 'local' -- the target spin is first passed through
 * ttup_transform_rotationaxes(rotation, r_world) (train.py:123-124; no gradient flows into it).  flags bit 1: check the mask's
 * format as ttup_uplift_forward's check_mask does -- the reference's training step goes through model.forward, which raises
 * unless the mask holds 0 and 1, both present, and nothing else (model.py:541-546): TTUP_EMASK otherwise (an all-ones or all-zeros
 * batch, a value such as 0.5, the additive {-1e9, 0} form).  The check costs one word read back and one stream synchronisation
 * after the pass is enqueued, so a call refused with TTUP_EMASK HAS written grad, loss, rot and pos: they hold no defined values
 * (loss_pos of an all-zeros mask is 0 / 0) and must not be used.  Without bit 1 nothing is checked, the call does not synchronise,
 * and the results are the same bits.  Every other refusal (TTUP_EINVAL: a null pointer, an unsupported variant, len outside
 * [1,255], 'local' with len 1, time_rotation 'old' with len above the handle's max_len, unknown flag bits, a workspace that is
 * too small or not 16-byte aligned) comes before anything is enqueued and leaves every output untouched.  Outputs (device): grad
 * (n_floats), loss[2] = {loss_rot, loss_pos}, rot (B,3), pos (B,T,3).  len <= 255.  No floating-point atomics: two calls on the
 * same inputs return the same bits, whatever the handle's max_batch.  A padded time step (mask 0) or an invisible keypoint
 * contributes exactly zero to every output but its own rows of pos. */
int    ttup_uplift_grad_layout(ttup_uplift* net, long long* n_floats, int* n_tensors, long long* offsets_host, int* used_host, int capacity);
size_t ttup_uplift_grad_workspace_bytes(ttup_uplift* net, int batch, int len);
int    ttup_uplift_loss_grad(ttup_uplift* net, const float* ball_dev, const float* table_dev, const float* mask_dev, const float* times_dev,
                             const float* r_world_dev, const float* rotation_dev, int batch, int len, int flags, void* workspace,
                             size_t workspace_bytes, float* grad_dev, float* loss_dev, float* rot_dev, float* pos_dev, void* stream);

/* ---------------------------------------------------------------- uplift optimizer step: clip, Adam, EMA (csrc/uplift_opt.hip)
 * Replaces, for one batch, what uplifting/train.py:129-132 does after loss.backward():
 *   torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm); optimizer.step() (torch.optim.Adam, no weight decay, no amsgrad);
 *   model_ema = update_ema(model, model_ema, ema_decay).
 *
 * ttup_opt_flat_step: the raw step on flat device buffers of any length.  param, m (exp_avg), v (exp_avg_sq), ema: n floats each,
 * updated in place; grad: n + hole_len floats, read only.  Element i of the four pairs with gradient element
 * i + (i >= hole_begin ? hole_len : 0), 0 <= hole_begin <= n: the relation between a handle's plain weights and the gradient layout,
 * whose embed.* block the plain weights lack.  The hole's gradient entries count towards the norm (the layout holds zeros there)
 * and touch no parameter.  step: the 1-based count of this step (bias corrections and step size are computed from it on the host in
 * double, as torch.optim.Adam does).  scratch: ttup_opt_flat_scratch_bytes() bytes, 8-byte aligned, private to the call while it
 * runs.  norm_out (nullable): receives the gradient's total L2 norm before clipping, one float.  Buffers must be 4-byte aligned;
 * 16-byte aligned ones are accessed 16 bytes at a time.  Three launches on `stream`, no synchronisation:
 *   norm = sqrt(sum g^2) with fp64 partial sums in a fixed tree;  c = min(1, max_norm / (norm + 1e-6));  g = c g;
 *   m += (1 - beta1) (g - m);  v = v beta2 + (1 - beta2) g g;  denom = sqrt(v) / sqrt(1 - beta2^step) + eps;
 *   param += -(lr / (1 - beta1^step)) m / denom;  ema = ema_decay ema + (1 - ema_decay) param
 * in fp32, in the operation order of torch's own kernels.  No floating-point atomics: two calls on equal inputs return equal bits.
 * A non-finite gradient propagates as in torch (error_if_nonfinite=False).
 *
 * ttup_uplift_opt_create: optimizer state for the weights of a 'connectstage' / 'dynamic' handle (any other variant: TTUP_EINVAL
 * before a device is touched): m and v zero, ema a copy of the weights (train.py:58), step count 0.  The handle must outlive it.
 * ttup_uplift_opt_step: one step on the handle's plain fp32 weights -- the weights ttup_uplift_loss_grad reads, so gradients ->
 * step -> gradients is consistent -- from grad_flat_dev, the buffer ttup_uplift_loss_grad filled (ttup_uplift_grad_layout).  The
 * handle's PACKED weights, which ttup_uplift_forward reads, are not updated: from the first step on the handle is marked trained
 * and ttup_uplift_forward on it returns TTUP_ESTALE without running.  To serve trained weights, read them back
 * (ttup_uplift_opt_read) and create a new handle from them (uplift.UpliftTrainer.model).
 * ttup_uplift_opt_read / _load: copy one of the four buffers (TTUP_OPT_*) to / from a caller-allocated device buffer in
 * gradient-layout order (ttup_uplift_grad_layout: n_floats entries); read writes zeros to the embed.* slots, load ignores them.
 * ttup_uplift_opt_set_step / _get_step: the number of steps taken so far (resume). */
#define TTUP_OPT_PARAM 0
#define TTUP_OPT_EMA   1
#define TTUP_OPT_M     2
#define TTUP_OPT_V     3
size_t ttup_opt_flat_scratch_bytes(void);
int    ttup_opt_flat_step(float* param_dev, const float* grad_dev, float* m_dev, float* v_dev, float* ema_dev, long long n, long long hole_begin,
                          long long hole_len, double lr, double beta1, double beta2, double eps, double ema_decay, double max_norm, long long step,
                          void* scratch_dev, float* norm_out_dev, void* stream);
int    ttup_uplift_opt_create(ttup_uplift* net, double lr, double beta1, double beta2, double eps, double ema_decay, double max_norm, ttup_uplift_opt** out);
void   ttup_uplift_opt_destroy(ttup_uplift_opt* opt);
int    ttup_uplift_opt_step(ttup_uplift_opt* opt, const float* grad_flat_dev, float* norm_out_dev, void* stream);
int    ttup_uplift_opt_read(ttup_uplift_opt* opt, int which, float* out_dev, void* stream);
int    ttup_uplift_opt_load(ttup_uplift_opt* opt, int which, const float* in_dev, void* stream);
int    ttup_uplift_opt_set_step(ttup_uplift_opt* opt, long long step);
int    ttup_uplift_opt_get_step(ttup_uplift_opt* opt, long long* step_host);

/* ---------------------------------------------------------------- a7: spin frame change
 * Replaces transform_rotationaxes (uplifting/helper.py:394-420): rot (B,3), pos (B,T,3) -> out (B,3). */
int ttup_transform_rotationaxes(const float* rot_dev, const float* pos_dev, int batch, int len, float* out_dev, void* stream);

/* ---------------------------------------------------------------- a7e: evaluation metrics (csrc/uplift_eval.hip)
 * The per-batch arithmetic of the reference's val (uplifting/train.py:166-195) and val_real (:250-283) over a whole prediction
 * set of n samples with t time steps: fp32 inputs, every per-sample operation and every sum in fp64, a fixed summation tree, no
 * floating-point atomics -- two calls return the same bits.  No handle; nothing synchronises with the host.  workspace:
 * ttup_uplift_eval_workspace_bytes(n) bytes (one query serves both calls), 8-byte aligned, private to the call while it runs.
 * Null pointers, n <= 0, t < 2 (the local frame is built from time steps 0 and 1) and a short workspace: TTUP_EINVAL before
 * any device call.  transform_global != 0: the predicted spin is in the world frame and is taken into the ball-local frame first.
 * A time step with mask == 0 is selected out (a non-finite value there is inert); the cosine is clamped to [-1, 1] before acos.
 *
 * ttup_uplift_val_metrics: pred_rot (n,3), pred_pos (n,t,3), r_world (n,t,3), rotation (n,3), mask (n,t).  The target spin goes
 *   through transform_rotationaxes(rotation, r_world), the predicted one too when transform_global.
 *   sums_dev[8]: over the samples, ||d||, |dx|, |dy|, |dz|, | ||pred|| - ||gt|| |, the angle in degrees, the masked mean position
 *     error sum_t ||pos - r_world|| mask / sum_t mask, and ||d||^2 (d = local predicted - local target spin).
 *   counts_dev[13]: TP[3], TN[3], FP[3], FN[3] per spin component, then n.  They are helper.binary_metrics called as the
 *     reference calls it (train.py:181), prediction first: TP both > 0, TN both < 0, FP prediction < 0 and target > 0,
 *     FN prediction > 0 and target < 0 -- FP and FN swapped relative to their names.
 * ttup_uplift_val_real_metrics: r_img (n,t,2) normalised image coordinates, Mint (n,3,3), Mext (n,4,4) row major, spin_class (n)
 *   int32 (1 topspin, 2 backspin, anything else: not annotated).  With transform_global the predicted spin goes through
 *   transform_rotationaxes(pred_rot, pred_pos) -- the PREDICTED positions (train.py:253).
 *   sums_dev[1]: over the samples, the masked mean distance between cam2img(world2cam(pred_pos, Mext), Mint) and
 *     r_img * (2560, 1440) (uplifting/helper.py:26) in pixels.
 *   counts_dev[5]: TP, TN, FP, FN of the sign of local spin component 1 against spin_class (train.py:265-276), then n.
 *   scores_dev[n]: local spin component 1 of every sample; labels_dev[n]: 1 topspin, 0 backspin, -1 not annotated. */
size_t ttup_uplift_eval_workspace_bytes(int n);
int    ttup_uplift_val_metrics(const float* pred_rot_dev, const float* pred_pos_dev, const float* r_world_dev, const float* rotation_dev, const float* mask_dev,
                               int n, int t, int transform_global, void* workspace_dev, size_t workspace_bytes, double* sums_dev, long long* counts_dev,
                               void* stream);
int    ttup_uplift_val_real_metrics(const float* pred_rot_dev, const float* pred_pos_dev, const float* r_img_dev, const float* mask_dev, const float* mint_dev,
                                    const float* mext_dev, const int* spin_class_dev, int n, int t, int transform_global, void* workspace_dev,
                                    size_t workspace_bytes, double* sums_dev, long long* counts_dev, double* scores_dev, int* labels_dev, void* stream);

/* ---------------------------------------------------------------- a3e: detector evaluation (csrc/detect_eval.hip)
 * What the reference's ball and table val() (balldetection/train.py:144-245, tabledetection/train.py:131-201) and its inference
 * scripts compute from heatmaps and positions: fp32 heatmaps and positions, fp64 centres, every operation and sum in fp64, a
 * fixed summation tree, no floating-point atomics -- two calls return the same bits.  No handle; nothing synchronises with the
 * host.  Workspaces are 8-byte aligned and private to the call while it runs.  Null pointers, n <= 0, sigma <= 0, an empty
 * tolerance list (or more than TTUP_DETECT_MAX_TOLERANCES) and a short workspace: TTUP_EINVAL before any device call.
 *
 * ttup_detect_heatmap_loss: pred (n,c,h,w); centres (n,c,2) [x, y] in output pixels; has_target (n,c) int32.
 *   sums_dev[n*c]: over the out_h x out_w output pixels, weight * (up(pred) - target)^2 with up = torch's bilinear interpolate
 *   (align_corners=False, no antialiasing: source coordinate (dst + 0.5) in/out - 0.5 clamped at 0, upper neighbour clamped at the
 *   last row / column; h, w may exceed the output), target = float32(exp(-((x-cx)^2 + (y-cy)^2) / (2 sigma^2))) or zeros where
 *   has_target is 0, weight = 100 where weighted and target > 0.1f, else 1 (weighted_mse_loss; weighted = 0: nn.MSELoss).
 *   Two source rows must fit the 60 KB of LDS a workgroup keeps them in: w <= 7680, else TTUP_EINVAL.
 * ttup_detect_heatmap_loss_grad: the same inputs and the same up, target and weight; writes the gradient of
 *   scale * sum over maps and output pixels of weight * (up(pred) - target)^2 with respect to pred,
 *     grad_dev[m, i, j] = float32(scale * sum_y sum_x 2 weight(y,x) (up(pred)[m,y,x] - target[m,y,x]) a_y(i) b_x(j)),
 *   a_y(i) the weight with which output row y reads source row i (1 - lambda on y0, lambda on y1, their sum where the clamp makes
 *   y0 == y1), b_x(j) the same for columns; fp64, rounded once on the store; a source row or column no output pixel reads gets +0.0.
 *   scale = 1 / (n c out_h out_w): the reference's loss.backward() into the network's output, before F.interpolate.  A gather: each
 *   source pixel is summed by one thread in a fixed order (two calls return the same bits), and nothing of the output resolution is
 *   written to device memory.  sums_dev (n*c, may be null: no sums wanted) receives what ttup_detect_heatmap_loss writes for the
 *   same inputs, bit for bit.  TTUP_EINVAL also for a non-finite scale; the width limit is the loss pass's (w <= 7680),
 *   whether sums are asked for or not.  ttup_detect_loss_grad_workspace_bytes: the workspace of both passes (0 for an empty shape).
 * ttup_detect_ball_metrics: pred_pos (n,3) [x, y, visibility]; gt, gt_min, gt_max (n,2); vis (n) int32.  Over the samples with
 *   vis == 1 (train.py:207-220):
 *   sums_dev[2]: over those with a detection (x, y > -100), the distance to gt, and the distance to the streak as val() measures
 *     it (distance_to_streak called with (pred, gt, gt_min, gt_max): the segments gt -> gt_min and gt_min -> gt_max).
 *   counts_dev[4 + n_tolerances]: visible samples; of those, pred visibility == 1 (PCK's denominator); of those, detected; per
 *     tolerance, pred visibility == 1 and within it of the nearer of the segments gt_min -> gt, gt -> gt_max
 *     (_batched_distance_point_to_segment: t = 0 where L^2 <= 1e-12, t clamped to [0, 1]); last, n.
 * ttup_detect_table_metrics: pred_pos, gt (n,keypoints,3) [x, y, visibility].  valid: pred visibility == 1; visible: gt's == 1.
 *   sums_dev[2]: the distance over valid & visible; unused.
 *   counts_dev[4 + n_tolerances]: valid; valid & visible; unused; per tolerance, valid & visible within it; last, n * keypoints. */
#define TTUP_DETECT_MAX_TOLERANCES 8
size_t ttup_detect_loss_workspace_bytes(int n_maps, int out_h, int out_w);
size_t ttup_detect_metrics_workspace_bytes(int n_items);
int    ttup_detect_heatmap_loss(const float* pred_dev, const double* centres_dev, const int* has_target_dev, int n, int c, int h, int w, double sigma, int out_h,
                                int out_w, int weighted, void* workspace_dev, size_t workspace_bytes, double* sums_dev, void* stream);
size_t ttup_detect_loss_grad_workspace_bytes(int n_maps, int h, int w, int out_h, int out_w);
int    ttup_detect_heatmap_loss_grad(const float* pred_dev, const double* centres_dev, const int* has_target_dev, int n, int c, int h, int w, double sigma, int out_h,
                                     int out_w, int weighted, double scale, void* workspace_dev, size_t workspace_bytes, double* sums_dev, float* grad_dev,
                                     void* stream);
int    ttup_detect_ball_metrics(const float* pred_pos_dev, const float* gt_dev, const float* gt_min_dev, const float* gt_max_dev, const int* vis_dev, int n,
                                const double* tolerances, int n_tolerances, void* workspace_dev, size_t workspace_bytes, double* sums_dev,
                                long long* counts_dev, void* stream);
int    ttup_detect_table_metrics(const float* pred_pos_dev, const float* gt_dev, int n, int keypoints, const double* tolerances, int n_tolerances,
                                 void* workspace_dev, size_t workspace_bytes, double* sums_dev, long long* counts_dev, void* stream);

/* ---------------------------------------------------------------- f2: synthetic-trajectory generator (BASELINE config 5)
 * Replaces the per-seed work of find_valid_trajectories_worker (syntheticdataset/mujocosimulation.py:112-219):
 *   ttup_trajgen_simulate  = _init_simulation (:54-109, CPython random.Random(seed) reproduced bit for bit) + the
 *                            mj_step sampling loop with its out-of-bounds / out-of-image stops (:112-151);
 *   ttup_trajgen_select    = _count_hits (helper.py:282-321) + every rejection and cut rule (:152-219).
 * mode: 0 final_lose, 1 final_win, 2 intermediate, 3 first_good, 4 first_short, 5 first_long (OOB_DEFINITIONS order);
 * direction: 0 left_to_right, 1 right_to_left.  substeps = RK4 steps per 1 ms MuJoCo timestep.
 * cam_host: 25 doubles on the HOST, Mext (4x4 row major) then Mint (3x3), as _calc_cammatrices builds them.
 * samples_dev: [n_labels][9][n_seeds] doubles (x y z vx vy vz wx wy wz; n_labels = ttup_trajgen_max_samples());
 * n_saved_dev: valid samples per seed.  init_dev (optional): [9][n_seeds] initial states.
 * n_keep_dev: 0 = rejected, else the number of samples the reference keeps; bounces_dev [n_seeds][4], n_bounces_dev.
 * The fluid / contact arithmetic restates MuJoCo's documented model (MuJoCo itself is not available): parity unpinned. */
int    ttup_trajgen_max_samples(void);
size_t ttup_trajgen_workspace_bytes(int n_seeds);
int ttup_trajgen_simulate(const int64_t* seeds_dev, int n_seeds, int mode, int direction, int substeps, const double* cam_host,
                          double* samples_dev, int* n_saved_dev, double* init_dev, void* workspace, size_t workspace_bytes, void* stream);
int ttup_trajgen_select(const double* samples_dev, const int* n_saved_dev, int n_seeds, int mode, int direction,
                        int* n_keep_dev, double* bounces_dev, int* n_bounces_dev, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- f4: camera calibration (csrc/calib.hip)
 * Replaces calibrate_camera (inference/utils.py:312-329 -> dataprocessing/regress_cameramatrices.py:199-231 with
 * use_ransac=True, dataprocessing/my_dlt.py) behind TableDetector.calibrate_camera / TableTennisPipeline.calibrate_camera
 * (interface.py:174-175, :291-299).  One workgroup per camera: DLT start, one lane per RANSAC subset, refinement on the inliers.
 * keypoints (B,13,3) float64 [x, y, visibility]; subsets (B,n_subsets,4) int32: the keys (1..13) drawn per RANSAC iteration
 * (keypoints 10 and 11 are added to every subset on the device); img_w/img_h: the principal point is fixed at (w//2, h//2).
 * Outputs: mint (B,3,4), mext (B,4,4) float64 row-major, n_inliers (B), status (B): 0 ok, -1 fewer than 6 visible keypoints,
 * -2 degenerate DLT start, -3 no inliers; start (B,8) the DLT start (fx, fy, t, euler xyz), nullable (tests). */
int ttup_calib_forward(const double* keypoints_dev, const int* subsets_dev, int batch, int n_subsets, int img_w, int img_h, int max_iter,
                       double* mint_dev, double* mext_dev, int* n_inliers_dev, int* status_dev, double* start_dev, void* stream);

/* ---------------------------------------------------------------- g1: drag + Magnus ODE fit (extension; csrc/odefit.hip)
 * BASELINE.json north_star names a "batched RK4 + Jacobian/Gauss-Newton" fit of flight dynamics to the detected 2-D track.
 * The reference has NO such code (its uplift is the transformer above): these entry points replace nothing and
 * are never called by the drop-in surface; parity is unpinned, validation is by self-consistency.
 * All arrays float64 on the device.  obs_xy (B,T,2) pixels; times (B,T) seconds, non-decreasing; mask (B,T) 0/1 or null;
 * cam: (B or 1, 21) = rows 0..2 of Mext (world -> camera, 12 numbers) then Mint (9), one per trajectory when cam_per_traj != 0;
 * init (B,9) starting point (r0 [m], v0 [m/s], w0 [rad/s] at times[:,0]).  Outputs: params (B,9), pos3d (B,T,3) at the time
 * stamps, cost (B) mean squared reprojection error [px^2], iters (B) accepted Levenberg-Marquardt steps (nullable except params).
 * h_max: largest RK4 step; an interval between two time stamps is cut into ceil(dt / h_max) equal steps. */
int ttup_odefit_forward(const double* obs_xy_dev, const double* times_dev, const double* mask_dev, const double* cam_dev, int cam_per_traj,
                        const double* init_dev, int batch, int len, double h_max, int max_iter, double tol,
                        double* params_dev, double* pos3d_dev, double* cost_dev, int* iters_dev, void* stream);
/* forward model only: params (B,9) -> pos3d (B,T,3) and / or pixels px (B,T,2) (either may be null) */
int ttup_odefit_integrate(const double* params_dev, const double* times_dev, const double* cam_dev, int cam_per_traj, int batch, int len,
                          double h_max, double* pos3d_dev, double* px_dev, void* stream);

/* ---------------------------------------------------------------- uplift training samples from generated trajectories (csrc/dataset.hip)
 * Replaces uplifting/data.py::TableTennisDataset.__getitem__ (:77-166, sample_camera :168-223) and the train transforms of
 * uplifting/transformations.py::get_transforms (:286-300), in the reference's order, fp64, cast to float32 at the end.
 * One sample = one (trajectory index, sample seed) pair; sample seed s reproduces `random.seed(s); np.random.seed(s); dataset[i]`
 * (0 <= s < 2^32, np.random.seed's range).  Call ttup_dataset_seed, then ttup_dataset_build with the same n and workspace.
 *   rows_dev (R,9) float64 packed trajectories (position, velocity, rotation), offsets_dev (V+1) int64, bounces_dev (V,4),
 *   n_bounces_dev (V) int32, times_dev (n_times) the shared time labels; mext_dev (V or 1, 4x4), mint_dev (V or 1, 3x3) the stored
 *   camera ('test' mode; cam_per_traj != 0: one per trajectory; may be null in 'train' mode).
 *   traj_index_host (n) int64 and seeds_host (n) int64 are HOST arrays (checked before anything is launched).
 *   mode: 0 train, 1 test (fps 50, stored camera, NormalizeImgCoords only).
 *   strengths_host[6]: blur_strength, randomize_std, stop_prob, randdet_prob, randmiss_prob, tablemiss_prob.
 *   transform_mask: bit k switches transform k on (MotionBlur, RandomizeDetections, RandomStop, RandomDetection, RandomMissing,
 *   TableMissing; bit 6: NormalizeImgCoords, the only one 'test' mode looks at); a cleared bit is the reference's Identity in that
 *   place (its numpy draws are skipped).
 *   out32_host / out64_host: HOST arrays of nine DEVICE pointers -- r_img (n,50,2), table_img (n,13,3), mask (n,50), r_world (n,50,3),
 *   rotation (n,3), times (n,50), bounces (n,1), Mint (n,3,3), Mext (n,4,4) -- float32 / float64; either set may be null, not both.
 *   diag_dev (n,4) int32: fps, n_frames (before the crop to 50), camera_tries, camera_success (fps -1: bad offsets, zeros written).
 *   record_dev (n,150) int32 or null (tests): per frame slot the nearest stored sample, the MotionBlur sample, the RandomMissing drop.
 * ttup_dataset_draws (tests): the next `count` raw MT19937 words of stream `which` (0 CPython random, 1 numpy) of every seeded
 * sample, out_dev (n,count) uint32; it advances the states, so seed again before a build. */
size_t ttup_dataset_workspace_bytes(int n);
int ttup_dataset_seed(const int64_t* seeds_host, int n, void* workspace, size_t workspace_bytes, void* stream);
int ttup_dataset_draws(void* workspace, size_t workspace_bytes, int n, int which, int count, uint32_t* out_dev, void* stream);
int ttup_dataset_build(const double* rows_dev, const int64_t* offsets_dev, int64_t n_rows, int n_traj, const double* bounces_dev,
                       const int* n_bounces_dev, const double* times_dev, int n_times, const double* mext_dev, const double* mint_dev,
                       int cam_per_traj, const int64_t* traj_index_host, int n, int mode, const double* strengths_host,
                       unsigned transform_mask, void* const* out32_host, void* const* out64_host, int* diag_dev, int* record_dev,
                       void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTUP_H */
