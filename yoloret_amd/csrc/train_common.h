// What the training files (headtrain.hip, convgrad.hip, bntrain.hip) share: their conventions, stated here once, and the rules that
// more than one of them applies.
//
// Conventions.  float32 only, wave64.  Rows are row-major over pixels, [pixels][ld] with the channel the fastest index, C <= ld
// channels taken, and only 4-byte aligned (a dense 75-float row), so every global access is a dword.  No float atomics, nothing in a
// workspace is read before the same call wrote it, every output element the contract names is written and nothing else (pad columns
// [C, ld) of a row are neither read nor written), and every chunk size is a function of the sizes only - never of the device, the CU
// count or a tuner: the same call gives the same bytes.  The files are compiled with -ffp-contract=off: every fused multiply-add is an
// explicit fmaf / MFMA, everything else is one IEEE float32 operation, in the order written.  Matrix products run on the float32
// matrix pipe (v_mfma_f32_16x16x4_f32: float32 operands and accumulation; headtrain.hip says why).  A sum over pixels is two-stage:
// workgroups own contiguous chunks and write one partial slab each to the workspace, the slabs are then added in index order.
#pragma once
#include "yr_common.h"
#include <limits.h>

#define TC_MAX_T 5          // 16-wide tiles per wave (workgroup) and side of the 1x1 kernels: 5 x 5 accumulators = 100 VGPRs

typedef float tc_f4 __attribute__((ext_vector_type(4)));      // an MFMA accumulator tile's four rows of a lane

// pixels * ld elements, as a byte offset, stay below 2^63
static inline bool tc_rows_fit(long long pixels, int ld) { return pixels <= (LLONG_MAX / 4) / ld; }

// the activations that have a derivative here
static inline bool tc_act_ok(int act) { return act == YR_ACT_NONE || act == YR_ACT_RELU6 || act == YR_ACT_SWISH; }

// n channels = tiles of 16 -> (blocks over the grid, tiles per block <= TC_MAX_T)
static inline void tc_blocking(int n, int* blocks, int* per) {
    const int t = (n + 15) / 16;
    *blocks = (t + TC_MAX_T - 1) / TC_MAX_T;
    *per = (t + *blocks - 1) / *blocks;
}

// the chunk rule: n items in chunks of at least `least`, and of as many more as keep the slabs at `most_slabs`
static inline long long tc_chunk(long long n, long long least, long long most_slabs) {
    const long long c = (n + most_slabs - 1) / most_slabs;
    return c < least ? least : c;
}

// the workspace an entry was given against the bytes its sizes need (0: sizes outside the contract)
static inline int tc_workspace_check(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
    YR_REQUIRE(workspace && need && workspace_bytes >= need, "%s: workspace null or of %zu bytes, %zu needed", who, workspace_bytes, need);
    YR_REQUIRE(((uintptr_t)workspace) % 16 == 0, "%s: workspace not 16-byte aligned", who);
    return YR_OK;
}

// Stage 2 of a two-stage sum (defined in headtrain.hip, one kernel for the library): out[e] = slab_0[e] + slab_1[e] + ... in index
// order, the first term slab_0[e] itself, for the n = rows * row_len elements of a slab; columns [row_valid, row_len) of every row
// are written as +0 and not read.  Every element of out is written.
int yr_launch_slab_sum(const float* slabs, int nchunks, int rows, int row_len, int row_valid, float* out, hipStream_t s);

#ifdef __HIPCC__
// The activations' derivatives, in pieces: a caller that multiplies further (a frozen scale) keeps its select around the whole
// product, so that the value outside ReLU6's interval is +0 whatever the factor.
// TensorFlow's Relu6Grad: 1 on the open interval 0 < u < 6, both ends strict
__device__ __forceinline__ bool tc_relu6_open(float u) { return u > 0.0f && u < 6.0f; }

// Swish'(u) = sg * (1 + u * (1 - sg)), sg = yr_sigmoid(u), four float32 operations in this order
__device__ __forceinline__ float tc_swish_grad(float u) {
    const float sg = yr_sigmoid(u);
    const float t1 = 1.0f - sg;
    const float t2 = u * t1;
    const float t3 = 1.0f + t2;
    return sg * t3;
}
#endif
