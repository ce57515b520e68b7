// The evaluation units' fixed-order reduction (csrc/detect_eval.hip, csrc/uplift_eval.hip), written once: fp64 sums and integer
// counts whose tree depends on the problem size alone -- no floating-point atomics, so two calls return the same bits.
//
//   lanes (xor butterfly) -> the block's waves / samples in order (one partial per block and quantity, in the workspace)
//   -> a final block per quantity: thread i adds the partials i, i + 256, ... in order, then a 256-leaf tree in LDS.
//
// Include after common.h, inside the unit's no_packed_fp32 bracket.
#pragma once

namespace ttup {

constexpr int ER_THREADS = 256;          // threads of a block that reduces: the tree's leaves

// xor butterfly over N neighbouring lanes (N = 64: the wave; 16: a quarter wave): every lane ends with the sum
template <int N, typename T>
__device__ __forceinline__ T lanes_sum(T v) {
#pragma unroll
    for (int off = N / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// per quantity the block's J values (one per wave / per sample, in LDS, behind a barrier), added in order -> the block's partial of
// that quantity: sums by the threads 0 .., counts by the threads 64 .. (another wave)
template <int NS, int NC, int J>
__device__ __forceinline__ void store_block_partials(const double (&sm)[NS][J], const int (&sc)[NC][J], int ncounts, long long nblocks, double* __restrict__ psum,
                                                     int* __restrict__ pcnt) {
    const int tid = ttup_tid_x();
    const long long blk = ttup_bid_x();
    if (tid < NS) {
        double v = 0.0;
        for (int k = 0; k < J; ++k) v = v + sm[tid][k];
        psum[(long long)tid * nblocks + blk] = v;
    } else if (tid >= 64 && tid < 64 + ncounts) {
        const int q = tid - 64;
        int v = 0;
        for (int k = 0; k < J; ++k) v += sc[q][k];
        pcnt[(long long)q * nblocks + blk] = v;
    }
}

// the whole block: thread i adds p[i], p[i + 256], ... in order, then a 256-leaf tree in sm[ER_THREADS] -> the total, in every thread
template <typename T, typename P>
__device__ __forceinline__ T block_tree_sum(const P* __restrict__ p, long long n, T* sm) {
    const int tid = ttup_tid_x();
    T acc = 0;
    for (long long i = tid; i < n; i += ER_THREADS) acc = acc + p[i];
    sm[tid] = acc;
    __syncthreads();
    for (int off = ER_THREADS / 2; off >= 1; off >>= 1) {
        if (tid < off) sm[tid] = sm[tid] + sm[tid + off];
        __syncthreads();
    }
    return sm[0];
}

// one block per quantity (nsums + ncounts blocks): its per-block partials in fixed order; counts[ncounts] = n
static __global__ __launch_bounds__(ER_THREADS) void eval_final_kernel(const double* __restrict__ psum, const int* __restrict__ pcnt, long long nblocks, int nsums,
                                                                        int ncounts, long long n, double* __restrict__ sums, long long* __restrict__ counts) {
    __shared__ double sd[ER_THREADS];
    __shared__ long long sl[ER_THREADS];
    const int tid = ttup_tid_x(), q = ttup_bid_x();
    if (q < nsums) {
        const double s = block_tree_sum(psum + (long long)q * nblocks, nblocks, sd);
        if (tid == 0) sums[q] = s;
    } else {
        const long long s = block_tree_sum(pcnt + (long long)(q - nsums) * nblocks, nblocks, sl);
        if (tid == 0) counts[q - nsums] = s;
    }
    if (q == 0 && tid == 0) counts[ncounts] = n;
}

// a metrics launch's workspace: per block nsums doubles, then (behind all doubles) its counts' ints
struct EvalPartials {
    double* psum;
    int* pcnt;
};

inline EvalPartials eval_partials(void* workspace, long long nblocks, int nsums) {
    double* psum = (double*)workspace;
    return {psum, (int*)(psum + nblocks * nsums)};
}

inline int eval_finish(const EvalPartials& p, long long nblocks, int nsums, int ncounts, long long n, double* sums, long long* counts, hipStream_t st) {
    hipLaunchKernelGGL(eval_final_kernel, dim3(nsums + ncounts), dim3(ER_THREADS), 0, st, (const double*)p.psum, (const int*)p.pcnt, nblocks, nsums, ncounts, n, sums, counts);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

}  // namespace ttup
