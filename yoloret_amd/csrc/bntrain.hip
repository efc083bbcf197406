// BatchNorm (+ activation) in training mode (reference yolo3/model.py:24-105: every convolution of the neck and the heads is followed by a
// BatchNormalization, momentum 0.9, epsilon 1e-3, and train.py calls the model with training=True): the forward pass on the statistics
// of the batch, the moving-average update, and the gradients for the input, gamma and beta.  yoloret_amd/autograd.py wires the two
// entries into torch.autograd; tests/bntrain_ref.py is the definition (TensorFlow's fused kernel and its gradient, restated).
//
// The conventions are those of train_common.h.  This file holds no fused multiply-add: every operation below is one IEEE float32
// operation, in the order written.
//
// Arithmetic (N = pixels):
//   mean = (sum_p z) / (float)N;  var = (sum_p (z - mean)^2) / (float)N, the deviations about the finished mean (a second read of z; never
//   E[z^2] - E[z]^2, never a merge of chunk moments);  invstd = 1 / sqrt(var + eps);  xhat = (z - mean) * invstd;
//   u = xhat * gamma + beta;  a = act(u);  moving_mean -= (moving_mean - mean) * (1 - momentum);
//   moving_var -= (moving_var - var * bessel) * (1 - momentum), bessel = (float)((double)N / (double)max(N - 1, 1)): the unbiased variance
//   that Keras' fused path stores.
//   backward: g = da * act'(u) (u and xhat recomputed by the forward's own operations: the same bits);  dbeta = sum_p g;
//   dgamma = sum_p (g * xhat);  dz = ((g - dbeta / N) - xhat * (dgamma / N)) * (gamma * invstd).
//
// Layout.  A workgroup of 1024 lanes owns a contiguous range of chunk = yr_bn_train_chunk(pixels, C) pixels and a block of Cb = min(C, 64)
// channels: lane t takes channel t % Cb and the pixels t / Cb, t / Cb + PP, ... of the range, PP = 1024 / Cb, so a wave's lanes run along
// the row (and across rows where C < 64: (pixel, channel) pairs flat over the lanes, fewer than Cb of the 1024 lanes idle).  A per-channel
// sum is two-stage: the lanes' partial sums (each from +0, in pixel order) are added in LDS in the order of t / Cb - for C >= 64 that is
// the wave order - and one [C] slab per chunk and sum goes to the workspace; the slabs are added in index order in the PROLOGUE of the
// next kernel, whose workgroups have the same shape: each adds the slabs of its own channels in the same order and gets the same bits
// (through LDS, BT_TILE slabs at a time: bt_slab_sum).  That is why the number of slabs is bounded by BT_MAX_CHUNKS = 256,
// not 1024 as CG_DW_MAX_CHUNKS: every workgroup reads all of them.
//   forward   3 launches: sums of z -> slabs;  [mean from the slabs] sums of (z - mean)^2 -> slabs, chunk 0 writes mean;
//             [var, invstd from the slabs] a = act(...), chunk 0 writes invstd and the moving statistics.
//   backward  2 launches: sums of g and g * xhat -> slabs;  [dbeta, dgamma from the slabs] dz, chunk 0 writes dgamma and dbeta.
//             With dz == null the second launch only adds the slabs.
#include "train_common.h"
#include <math.h>

#define BT_THREADS 1024         // lanes per workgroup: 16 waves, so that the at most 256 ranges of a map still fill the machine
#define BT_CB 64               // channels per workgroup, at most
#define BT_MIN_ELEMS 8192      // elements per stage-1 workgroup, at least (8 per lane)
#define BT_TILE 128            // slabs in LDS at a time when they are added (32 KB)
#define BT_MAX_CHUNKS 256      // slabs per sum, at most (1024 from 2^38 pixels on, where the chunk would not fit an int)

struct bt_geo {
    long long pixels, chunk;
    int C, Cb, PP, nchunks;
    float fn;      // (float)pixels
};

static inline bool bt_sizes_ok(long long pixels, int C) { return pixels >= 1 && pixels < (1ll << 40) && C >= 1 && C <= INT_MAX - BT_CB; }

static inline long long bt_chunk(long long pixels, int C) {
    const int cb = C < BT_CB ? C : BT_CB;
    return tc_chunk(pixels, (BT_MIN_ELEMS + cb - 1) / cb, pixels < (1ll << 38) ? BT_MAX_CHUNKS : 1024);
}

static inline bt_geo bt_make_geo(long long pixels, int C) {
    bt_geo g;
    g.pixels = pixels;
    g.chunk = bt_chunk(pixels, C);
    g.C = C;
    g.Cb = C < BT_CB ? C : BT_CB;
    g.PP = BT_THREADS / g.Cb;
    g.nchunks = (int)((pixels + g.chunk - 1) / g.chunk);
    g.fn = (float)pixels;
    return g;
}

extern "C" int yr_bn_train_chunk(long long pixels, int C) { return bt_sizes_ok(pixels, C) ? (int)bt_chunk(pixels, C) : 0; }

extern "C" size_t yr_bn_train_workspace_bytes(long long pixels, int C) {
    if (!bt_sizes_ok(pixels, C)) return 0;
    const bt_geo g = bt_make_geo(pixels, C);
    return (size_t)2 * (size_t)g.nchunks * (size_t)C * sizeof(float);
}

// what every kernel below knows about its lane: the channel (block blockIdx.x of Cb channels), its first pixel and the end of the range
struct bt_lane {
    int cl, po, c;
    bool on;
    long long p, p1;
};

__device__ __forceinline__ bt_lane bt_lane_of(const bt_geo& g) {
    bt_lane l;
    l.po = (int)threadIdx.x / g.Cb;
    l.cl = (int)threadIdx.x - l.po * g.Cb;
    l.c = (int)blockIdx.x * BT_CB + l.cl;
    l.on = l.po < g.PP && l.c < g.C;
    const long long p0 = (long long)blockIdx.y * g.chunk;
    l.p1 = p0 + g.chunk < g.pixels ? p0 + g.chunk : g.pixels;
    l.p = p0 + l.po;
    return l;
}

// the lanes' partial sums of one channel, added in the order of po; lane po = 0 of the channel writes the slab element
__device__ __forceinline__ void bt_fold(const bt_geo& g, const bt_lane& l, float acc, float* red, float* __restrict__ slab) {
    red[threadIdx.x] = acc;
    __syncthreads();
    if (l.po == 0 && l.c < g.C) {
        const float* col = red + l.cl;
        float v = 0.0f;
        int k = 0;
        for (; k + 16 <= g.PP; k += 16) {      // (sixteen LDS reads in flight, then their additions in order)
            float r[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) r[i] = col[(k + i) * g.Cb];
#pragma unroll
            for (int i = 0; i < 16; ++i) v = v + r[i];
        }
        for (; k < g.PP; ++k) v = v + col[k * g.Cb];
        slab[(size_t)blockIdx.y * g.C + l.c] = v;
    }
}

// The slabs [nchunks][C] of this workgroup's channel block, added in index order from +0: every lane of the workgroup helps to bring
// BT_TILE slabs at a time into LDS (rows of the block's channels, contiguous), then lane t < (channels of the block) adds channel t's
// column in order.  -> the sum in those lanes (0 in the others).  Every lane of the workgroup must call it (it holds barriers), and the
// workgroup has BT_THREADS lanes.  (One lane a channel walking the slabs in global memory with eight loads in flight, and a tile loaded
// with one load in flight, were both measured slower: DESIGN.md row f-10.)
__device__ __forceinline__ float bt_slab_sum(const float* __restrict__ slabs, const bt_geo& g, float* tile) {
    const int c0 = (int)blockIdx.x * BT_CB;
    const int cb = g.C - c0 < g.Cb ? g.C - c0 : g.Cb;
    float v = 0.0f;
    for (int j0 = 0; j0 < g.nchunks; j0 += BT_TILE) {
        const int nj = g.nchunks - j0 < BT_TILE ? g.nchunks - j0 : BT_TILE;
        float r[BT_TILE * BT_CB / BT_THREADS];      // all of a lane's loads of the tile in flight before the first LDS store
#pragma unroll
        for (int i = 0; i < BT_TILE * BT_CB / BT_THREADS; ++i) {
            const int e = i * BT_THREADS + (int)threadIdx.x;
            const int j = e / cb, cc = e - j * cb;
            r[i] = e < nj * cb ? slabs[(size_t)(j0 + j) * g.C + c0 + cc] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < BT_TILE * BT_CB / BT_THREADS; ++i) {
            const int e = i * BT_THREADS + (int)threadIdx.x;
            const int j = e / cb, cc = e - j * cb;
            if (e < nj * cb) tile[j * BT_CB + cc] = r[i];
        }
        __syncthreads();
        if ((int)threadIdx.x < cb) {      // sixteen LDS reads in flight, then their additions in order: one read at a time waits out its latency
            const float* col = tile + threadIdx.x;
            int j = 0;
            for (; j + 16 <= nj; j += 16) {
                float r[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) r[k] = col[(j + k) * BT_CB];
#pragma unroll
                for (int k = 0; k < 16; ++k) v = v + r[k];
            }
            for (; j < nj; ++j) v = v + col[j * BT_CB];
        }
        __syncthreads();
    }
    return v;
}

__device__ __forceinline__ float bt_invstd(float var, float eps) { return 1.0f / __builtin_sqrtf(var + eps); }

// g = da * act'(u)
__device__ __forceinline__ float bt_act_grad(float da, float u, int act) {
    if (act == YR_ACT_RELU6) return tc_relu6_open(u) ? da : 0.0f;
    if (act == YR_ACT_SWISH) return da * tc_swish_grad(u);
    return da;
}

// ---------------------------------------------------------------- forward
__global__ __launch_bounds__(BT_THREADS) void bt_sum_kernel(const float* __restrict__ z, long long z_ld, bt_geo g, float* __restrict__ slabs) {
    __shared__ float red[BT_THREADS];
    const bt_lane l = bt_lane_of(g);
    float acc = 0.0f;
    if (l.on) {
        const float* zp = z + l.c;
#pragma unroll 4
        for (long long p = l.p; p < l.p1; p += g.PP) acc = acc + zp[p * z_ld];
    }
    bt_fold(g, l, acc, red, slabs);
}

__global__ __launch_bounds__(BT_THREADS) void bt_sqdev_kernel(const float* __restrict__ z, long long z_ld, bt_geo g, const float* __restrict__ sums,
                                                             float* __restrict__ slabs, float* __restrict__ mean) {
    __shared__ float red[BT_THREADS];
    __shared__ float stat[BT_CB];
    __shared__ float tile[BT_TILE * BT_CB];
    const bt_lane l = bt_lane_of(g);
    const float total = bt_slab_sum(sums, g, tile);
    if (l.po == 0 && l.c < g.C) {
        const float m = total / g.fn;
        stat[l.cl] = m;
        if (blockIdx.y == 0) mean[l.c] = m;
    }
    __syncthreads();
    float acc = 0.0f;
    if (l.on) {
        const float m = stat[l.cl];
        const float* zp = z + l.c;
#pragma unroll 4
        for (long long p = l.p; p < l.p1; p += g.PP) {
            const float d = zp[p * z_ld] - m;
            acc = acc + d * d;
        }
    }
    bt_fold(g, l, acc, red, slabs);
}

__global__ __launch_bounds__(BT_THREADS) void bt_apply_kernel(const float* __restrict__ z, long long z_ld, bt_geo g, const float* __restrict__ sqdevs,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ mean, float eps, float momentum, float bessel, int act,
                                                             float* __restrict__ a, long long a_ld, float* __restrict__ invstd,
                                                             float* __restrict__ moving_mean, float* __restrict__ moving_var) {
    __shared__ float sm[BT_CB], si[BT_CB], sg[BT_CB], sb[BT_CB];
    __shared__ float tile[BT_TILE * BT_CB];
    const bt_lane l = bt_lane_of(g);
    const float total = bt_slab_sum(sqdevs, g, tile);
    if (l.po == 0 && l.c < g.C) {
        const float var = total / g.fn;
        const float is = bt_invstd(var, eps), m = mean[l.c];
        sm[l.cl] = m;
        si[l.cl] = is;
        sg[l.cl] = gamma[l.c];
        sb[l.cl] = beta[l.c];
        if (blockIdx.y == 0) {
            invstd[l.c] = is;
            if (moving_mean) {
                const float d = 1.0f - momentum;
                const float mm = moving_mean[l.c], mv = moving_var[l.c];
                const float dm = (mm - m) * d;
                const float dv = (mv - var * bessel) * d;
                moving_mean[l.c] = mm - dm;
                moving_var[l.c] = mv - dv;
            }
        }
    }
    __syncthreads();
    if (!l.on) return;
    const float m = sm[l.cl], is = si[l.cl], ga = sg[l.cl], be = sb[l.cl];
    const float* zp = z + l.c;
    float* ap = a + l.c;
#pragma unroll 4
    for (long long p = l.p; p < l.p1; p += g.PP) {
        const float xh = (zp[p * z_ld] - m) * is;
        const float t = xh * ga;
        ap[p * a_ld] = yr_apply_act(t + be, act);
    }
}

// ---------------------------------------------------------------- backward
__global__ __launch_bounds__(BT_THREADS) void bt_bwd_sums_kernel(const float* __restrict__ da, long long da_ld, const float* __restrict__ z, long long z_ld,
                                                                bt_geo g, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd, int act,
                                                                float* __restrict__ slabs_b, float* __restrict__ slabs_g) {
    __shared__ float red[BT_THREADS];
    const bt_lane l = bt_lane_of(g);
    float accb = 0.0f, accg = 0.0f;
    if (l.on) {
        const float m = mean[l.c], is = invstd[l.c], ga = gamma[l.c], be = beta[l.c];
        const float* zp = z + l.c;
        const float* dp = da + l.c;
#pragma unroll 4
        for (long long p = l.p; p < l.p1; p += g.PP) {
            const float xh = (zp[p * z_ld] - m) * is;
            const float t = xh * ga;
            const float gr = bt_act_grad(dp[p * da_ld], t + be, act);
            accb = accb + gr;
            accg = accg + gr * xh;
        }
    }
    bt_fold(g, l, accb, red, slabs_b);
    __syncthreads();      // red is read by the first fold's adders
    bt_fold(g, l, accg, red, slabs_g);
}

__global__ __launch_bounds__(BT_THREADS) void bt_bwd_apply_kernel(const float* __restrict__ da, long long da_ld, const float* __restrict__ z, long long z_ld,
                                                                 bt_geo g, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd, int act,
                                                                 const float* __restrict__ slabs_b, const float* __restrict__ slabs_g,
                                                                 float* __restrict__ dz, long long dz_ld, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta) {
    __shared__ float sm[BT_CB], si[BT_CB], sg[BT_CB], sb[BT_CB], smg[BT_CB], smgx[BT_CB];
    __shared__ float tile[BT_TILE * BT_CB];
    const bt_lane l = bt_lane_of(g);
    const float db = bt_slab_sum(slabs_b, g, tile), dg = bt_slab_sum(slabs_g, g, tile);
    if (l.po == 0 && l.c < g.C) {
        sm[l.cl] = mean[l.c];
        si[l.cl] = invstd[l.c];
        sg[l.cl] = gamma[l.c];
        sb[l.cl] = beta[l.c];
        smg[l.cl] = db / g.fn;
        smgx[l.cl] = dg / g.fn;
        if (blockIdx.y == 0) {
            dbeta[l.c] = db;
            dgamma[l.c] = dg;
        }
    }
    __syncthreads();
    if (!l.on) return;
    const float m = sm[l.cl], is = si[l.cl], ga = sg[l.cl], be = sb[l.cl], mg = smg[l.cl], mgx = smgx[l.cl];
    const float k = ga * is;
    const float* zp = z + l.c;
    const float* dp = da + l.c;
    float* op = dz + l.c;
#pragma unroll 4
    for (long long p = l.p; p < l.p1; p += g.PP) {
        const float xh = (zp[p * z_ld] - m) * is;
        const float t = xh * ga;
        const float gr = bt_act_grad(dp[p * da_ld], t + be, act);
        const float r1 = gr - mg;
        const float r2 = xh * mgx;
        op[p * dz_ld] = (r1 - r2) * k;
    }
}

// dz == null: only the slabs' sums, a workgroup per block of channels
__global__ __launch_bounds__(BT_THREADS) void bt_bwd_finish_kernel(bt_geo g, const float* __restrict__ slabs_b, const float* __restrict__ slabs_g,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ float tile[BT_TILE * BT_CB];
    const float db = bt_slab_sum(slabs_b, g, tile), dg = bt_slab_sum(slabs_g, g, tile);
    const int c = (int)blockIdx.x * BT_CB + (int)threadIdx.x;
    if ((int)threadIdx.x < g.Cb && c < g.C) {
        dbeta[c] = db;
        dgamma[c] = dg;
    }
}

// ---------------------------------------------------------------- entries
static int bt_check_common(const char* who, long long pixels, int C, int act, void* workspace, size_t workspace_bytes) {
    YR_REQUIRE(bt_sizes_ok(pixels, C), "%s: pixels must be 1..2^40-1 and C positive (pixels %lld, C %d)", who, pixels, C);
    YR_REQUIRE(tc_act_ok(act), "%s: act %d is not none, ReLU6 or Swish", who, act);
    return tc_workspace_check(who, workspace, workspace_bytes, yr_bn_train_workspace_bytes(pixels, C));
}

extern "C" int yr_bn_train_forward(const float* z, int z_ld, const float* gamma, const float* beta, long long pixels, int C, float eps, float momentum,
                                   int act, float* a, int a_ld, float* mean, float* invstd, float* moving_mean, float* moving_var, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    YR_REQUIRE(z && gamma && beta && a && mean && invstd, "bn_train_forward: null pointer");
    YR_REQUIRE((moving_mean != nullptr) == (moving_var != nullptr), "bn_train_forward: moving_mean and moving_var go together: both or neither");
    const int rc = bt_check_common("bn_train_forward", pixels, C, act, workspace, workspace_bytes);
    if (rc != YR_OK) return rc;
    YR_REQUIRE(eps >= 0.0f && eps < INFINITY, "bn_train_forward: eps must be finite and not negative (%g)", (double)eps);
    YR_REQUIRE(momentum >= 0.0f && momentum <= 1.0f, "bn_train_forward: momentum must lie in [0, 1] (%g)", (double)momentum);
    YR_REQUIRE(z_ld >= C && a_ld >= C, "bn_train_forward: a leading dimension below C = %d", C);
    YR_REQUIRE(tc_rows_fit(pixels, z_ld) && tc_rows_fit(pixels, a_ld), "bn_train_forward: byte offsets beyond 2^63");
    YR_REQUIRE(((uintptr_t)z | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)a | (uintptr_t)mean | (uintptr_t)invstd | (uintptr_t)moving_mean |
                (uintptr_t)moving_var) % 4 == 0, "bn_train_forward: pointer not 4-byte aligned");
    const bt_geo g = bt_make_geo(pixels, C);
    const float bessel = (float)((double)pixels / (double)(pixels > 1 ? pixels - 1 : 1));
    float* sums = (float*)workspace;
    float* sqdevs = sums + (size_t)g.nchunks * C;
    const dim3 grid((unsigned)((C + BT_CB - 1) / BT_CB), (unsigned)g.nchunks);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bt_sum_kernel, grid, dim3(BT_THREADS), 0, s, z, (long long)z_ld, g, sums);
    YR_LAUNCH_CHECK();
    hipLaunchKernelGGL(bt_sqdev_kernel, grid, dim3(BT_THREADS), 0, s, z, (long long)z_ld, g, (const float*)sums, sqdevs, mean);
    YR_LAUNCH_CHECK();
    hipLaunchKernelGGL(bt_apply_kernel, grid, dim3(BT_THREADS), 0, s, z, (long long)z_ld, g, (const float*)sqdevs, gamma, beta, (const float*)mean, eps,
                       momentum, bessel, act, a, (long long)a_ld, invstd, moving_mean, moving_var);
    YR_LAUNCH_CHECK();
    return YR_OK;
}

extern "C" int yr_bn_train_backward(const float* da, int da_ld, const float* z, int z_ld, const float* gamma, const float* beta, const float* mean,
                                    const float* invstd, long long pixels, int C, int act, float* dz, int dz_ld, float* dgamma, float* dbeta,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    YR_REQUIRE(da && z && gamma && beta && mean && invstd && dgamma && dbeta, "bn_train_backward: null pointer");
    const int rc = bt_check_common("bn_train_backward", pixels, C, act, workspace, workspace_bytes);
    if (rc != YR_OK) return rc;
    YR_REQUIRE(da_ld >= C && z_ld >= C && (!dz || dz_ld >= C), "bn_train_backward: a leading dimension below C = %d", C);
    YR_REQUIRE(tc_rows_fit(pixels, da_ld) && tc_rows_fit(pixels, z_ld) && (!dz || tc_rows_fit(pixels, dz_ld)), "bn_train_backward: byte offsets beyond 2^63");
    YR_REQUIRE(((uintptr_t)da | (uintptr_t)z | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)mean | (uintptr_t)invstd | (uintptr_t)dz |
                (uintptr_t)dgamma | (uintptr_t)dbeta) % 4 == 0, "bn_train_backward: pointer not 4-byte aligned");
    const bt_geo g = bt_make_geo(pixels, C);
    float* slabs_b = (float*)workspace;
    float* slabs_g = slabs_b + (size_t)g.nchunks * C;
    const dim3 grid((unsigned)((C + BT_CB - 1) / BT_CB), (unsigned)g.nchunks);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bt_bwd_sums_kernel, grid, dim3(BT_THREADS), 0, s, da, (long long)da_ld, z, (long long)z_ld, g, gamma, beta, mean, invstd, act, slabs_b,
                       slabs_g);
    YR_LAUNCH_CHECK();
    if (dz)
        hipLaunchKernelGGL(bt_bwd_apply_kernel, grid, dim3(BT_THREADS), 0, s, da, (long long)da_ld, z, (long long)z_ld, g, gamma, beta, mean, invstd, act,
                           (const float*)slabs_b, (const float*)slabs_g, dz, (long long)dz_ld, dgamma, dbeta);
    else
        hipLaunchKernelGGL(bt_bwd_finish_kernel, grid.x, dim3(BT_THREADS), 0, s, g, (const float*)slabs_b,
                           (const float*)slabs_g, dgamma, dbeta);
    YR_LAUNCH_CHECK();
    return YR_OK;
}
