// Device helpers shared by the convolution units (conv.hip and its kernel headers, conv_x3.hip, conv_f32.hip, peaks.hip): vector
// types, bf16 packing, LDS tile addressing, staging through registers, and the small idioms every tiled kernel repeats.
#pragma once
#include "common.h"

namespace ttup {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(2))) short s16x2;

// MI355X: 8 XCDs with a private L2 each, workgroups dealt to them round-robin by linear id.  Persistent kernels walk tiles
// t = blockIdx.x + it * gridDim.x (gridDim.x a multiple of 8), so tile t runs on XCD t % 8 and raster neighbours -- which share
// halo rows / columns -- sit behind eight different L2s.  This remaps the sequence so that every XCD walks one contiguous
// eighth of the raster order: neighbours' halos become hits in the XCD's own L2 (PMC: 1.51 -> 1.40 GB of L2 fills per frame).
// Not applied in conv_mfma_kernel: its HBM-bound full-resolution conv gets 5-10 % slower with eight widely separated streams.
__device__ __forceinline__ int xcd_tile(int t, int total) {
    const int main = total & ~7;
    return t < main ? (t & 7) * (main >> 3) + (t >> 3) : t;
}

// two fp32 -> packed bf16 pair, round-to-nearest-even in hardware (v_cvt_pk_bf16_f32)
// (as ONE vector conversion: two scalar casts come out as two conversions merged by a v_perm)
__device__ __forceinline__ unsigned pack2(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}

// ReLU on a packed bf16 pair: bf16 is sign-magnitude, so as int16 every negative value (and -0) is < 0 (v_pk_max_i16)
__device__ __forceinline__ unsigned relu_pk(unsigned p) {
    const s16x2 z = {0, 0};
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, p), z));
}

// LDS offset (in bf16 elements) of 8-channel group c8 of tile pixel (iy, ix).
// CK=32 (64 B per pixel): the 16-byte chunk index is XOR-swizzled with bits 1..2 of the tile column, which makes a
// 16-pixel ds_read_b128 conflict-free at every alignment (stride-1) and 2-way instead of 4-way at stride 2.
// CK=16 (32 B per pixel) is conflict-free as is.
template <int CK, int IW>
__device__ __forceinline__ int lds_off(int iy, int ix, int c8) {
    if (CK == 32) return ((iy * IW + ix) * 4 + (c8 ^ ((ix >> 1) & 3))) * 8;
    return ((iy * IW + ix) * (CK / 8) + c8) * 8;
}

// Copy UNITS 16-byte units from global memory into LDS with a 512-thread workgroup: every thread issues ALL of its loads before
// its first LDS store, i.e. one memory round trip for the block (a plain `for (u = tid; u < n; u += 512) dst[u] = src[u]` loop
// compiles to load / wait / store per iteration: UNITS / 512 serial round trips at the start of every persistent kernel).
template <int UNITS> struct StageRegs { u32x4 v[(UNITS + 511) / 512]; };
template <int UNITS>
__device__ __forceinline__ void stage_load_512(StageRegs<UNITS>& r, const bf16_t* src, int tid) {
#pragma unroll
    for (int k = 0; k < (UNITS + 511) / 512; ++k) { const int u = tid + k * 512; r.v[k] = u32x4{0u, 0u, 0u, 0u}; if (u < UNITS) r.v[k] = ((const u32x4*)src)[u]; }
}
template <int UNITS>
__device__ __forceinline__ void stage_store_512(bf16_t* dst, const StageRegs<UNITS>& r, int tid) {
#pragma unroll
    for (int k = 0; k < (UNITS + 511) / 512; ++k) { const int u = tid + k * 512; if (u < UNITS) ((u32x4*)dst)[u] = r.v[k]; }
}

// A 32-bit per-lane offset the compiler must treat as unknown HERE: its zero-extension then happens next to the load that uses it, and
// "uniform 64-bit base + zext(32-bit lane offset)" is selected as ONE global_load with a scalar base (saddr) and a 32-bit vector
// offset.  Without it the extension is hoisted out of the tile loop (a register PAIR per offset) and every load gets a 64-bit add.
__device__ __forceinline__ unsigned opaque_u32(unsigned v) { asm volatile("" : "+v"(v)); return v; }

// "These prefetched registers are needed HERE": an empty asm statement that takes them as inputs makes the compiler place its
// s_waitcnt for their loads at this point and treat them as complete afterwards.  The persistent kernels call it BEFORE an epilogue
// issues its stores: the vector-memory counter retires in order and the compiler cannot count stores that sit behind a branch, so a
// wait for prefetched loads that comes AFTER the stores is an s_waitcnt vmcnt(0) -- it drains the stores just issued, with every wave
// of the workgroup parked for a store round trip per tile (round 5: the stem spent 2.7 k of its 11.9 k cycles per tile there).
template <typename T, int N>
__device__ __forceinline__ void prefetch_arrived(const T (&r)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("" :: "v"(r[k]));
}

// ------------------------------------------------------------------ idioms of the tiled kernels
// Tile tl of a batch cut into TH x TW tiles, tiles_x per tile row: its image b and its first pixel (y0, x0) -- less PAD, for the
// origin of the halo tile a conv stages (a stride-S conv's input tile: TH * S, TW * S).
struct TileAt { int b, y0, x0; };
template <int TH, int TW, int PAD = 0>
__device__ __forceinline__ TileAt tile_at(int tl, int tiles_per_img, int tiles_x) {
    const int b = tl / tiles_per_img, t = tl % tiles_per_img;
    return TileAt{b, (t / tiles_x) * TH - PAD, (t % tiles_x) * TW - PAD};
}

// eight fp32 values (two accumulator quads, or v[0..7]) -> four packed bf16 pairs, with ReLU on the packed pairs when `relu`
__device__ __forceinline__ u32x4 pack8(f32x4 lo, f32x4 hi, bool relu) {
    u32x4 pk;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned w = i < 2 ? pack2(lo[2 * (i & 1)], lo[2 * (i & 1) + 1]) : pack2(hi[2 * (i & 1)], hi[2 * (i & 1) + 1]);
        pk[i] = relu ? relu_pk(w) : w;
    }
    return pk;
}
__device__ __forceinline__ u32x4 pack8(const float* v, bool relu) {
    u32x4 pk;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const unsigned w = pack2(v[2 * i], v[2 * i + 1]); pk[i] = relu ? relu_pk(w) : w; }
    return pk;
}

// v[0..7] += the eight bf16 values of rv (a residual / fuse-layer term as it lies in memory: four pairs, low half first)
__device__ __forceinline__ void add_bf16x8(float* v, u32x4 rv) {
    const unsigned w4[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[2 * k] += bf16_to_f32((bf16_t)(w4[k] & 0xffff)); v[2 * k + 1] += bf16_to_f32((bf16_t)(w4[k] >> 16)); }
}

// Fragment (k-step k, m-tile m) of a 1x1 follower 64 -> 16 * MT with its K order permuted to the accumulator layout of the 64-channel
// convs: a lane owns channels g*16 .. g*16+15 of its pixel, so k-step k takes channels 16g + 8k + j from lane group g -- the bf16 pairs
// it has just packed -- and the tile never goes through LDS.  In the standard packing those channels sit at k-step g>>1, lane group
// 2(g&1)+k.
template <int MT>
__device__ __forceinline__ bf16x8 follower_frag(const bf16_t* w, int k, int m, int n, int g) {          // lane = g * 16 + n
    return *(const bf16x8*)(w + (((g >> 1) * MT + m) * 64 + n + 16 * ((g & 1) * 2 + k)) * 8);
}

// ------------------------------------------------------------------ host side
// What every launcher does once its arguments are filled: raise the kernel's dynamic-LDS limit on this device, return on an empty
// grid, leave the kernel's template-id for the roofline (kernel_note: exactly as rocprofv3 prints it), launch, check.
template <typename Args, typename... Ids>
static int launch_noted(void (*kernel)(Args), dim3 grid, int threads, size_t smem, hipStream_t st, const Args& a, const char* id_fmt, Ids... ids) {
    if (int rc = ensure_max_lds((const void*)kernel, smem)) return rc;
    if (grid.x == 0 || grid.y == 0 || grid.z == 0) return TTUP_OK;
    if constexpr (sizeof...(Ids) == 0) kernel_note("%s", id_fmt);
    else kernel_note(id_fmt, ids...);
    hipLaunchKernelGGL(kernel, grid, dim3(threads), smem, st, a);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}
// grid of a persistent kernel: one workgroup per tile up to per_cu resident workgroups on each of the 256 CUs
static inline int persistent_grid(int total_tiles, int per_cu = 1) { return total_tiles < 256 * per_cu ? total_tiles : 256 * per_cu; }

}  // namespace ttup
