// The squeeze-excite block, forward and backward (reference yolo3/efficientnet.py:406-438: the mean over the map, a 1x1 convolution
// with bias to R channels, Swish, a 1x1 convolution with bias back to C channels, sigmoid, and the map multiplied by that gate; every
// MBConv of the EfficientNet backbones and of the six head blocks, yolo3/model.py:91-115, runs one with se_ratio 0.25).
// yoloret_amd/autograd.py wires the two entries into torch.autograd; tests/segrad_ref.py is the definition (the reference has no backward
// code of its own: TensorFlow's tape provides it).  The inference kernels (se_mean_kernel, se_fc_kernel, se_tail.h) live inside plans and
// keep nothing a backward needs; nothing of them is touched here.
//
// The conventions are those of train_common.h.  This file holds no fused multiply-add but those inside yr_sigmoid's pinned exp: every
// other operation below is one IEEE float32 operation, in the order written.  Maps are [B][H][W][ld], N = H * W pixels an image, C <= ld
// channels taken; w1 [C][R], b1 [R], w2 [R][C], b2 [C], m [B][C], z1 [B][R], g [B][C] are dense.
//
// The map passes (the hot path: two sums over the pixels and two element-wise passes, all memory-bound) share ONE layout.  The C channels
// are cut into nb = ceil(C / 64) blocks of Cb = ceil(C / nb) channels (96 channels: two blocks of 48, no half-empty block), an image's N
// pixels into contiguous ranges of chunk = yr_se_chunk(B, N, C) pixels.  A workgroup of SE_THREADS = 256 lanes owns one range of one image
// and one channel block: lane t takes channel t % Cb of the block and the pixels t / Cb, t / Cb + PP, ... of the range, PP = 256 / Cb, so
// the channel is the fastest index over the lanes and a wave reads row segments, a dword a lane (rows are only 4-byte aligned).  The
// (image, range) pairs are numbered u = b * nchunks + j and walked by blockIdx.x with a grid stride (one step for every size a device
// holds); blockIdx.y is the channel block.
//   a sum over the pixels (S = sum_p x, dg = sum_p dy * x) is two-stage.  Stage 1: a lane adds its terms in increasing p from +0 (for dg
//   each term one rounded product, added by one rounded addition); the lanes of a channel are added through LDS in the order of
//   t / Cb = 0 .. PP - 1 from +0; the result is element c of slab u, slabs [B][nchunks][C] in the workspace.  Stage 2 (in the small kernel
//   that follows): the slabs of an image in index order j = 0 .. nchunks - 1 from +0.  This is tests/bntrain_ref.ordered_sum per image.
//
// The small kernels (the two 1x1 convolutions on [B][C] vectors and their backward: 64 x 512 x 128 multiply-adds at most in the shipped
// models) run one workgroup of SE_FC_THREADS = 1024 lanes an image, the vectors in LDS.  Plain products and sums, no fmaf:
//   fc (a reduction over the ROWS of the matrix: z1 from w1 [C][R], z2 from w2 [R][C]; I inputs, O outputs)   OL = min(O, 1024),
//       KS = 1024 / OL slices of SL = ceil(I / KS) inputs.  Lane t = k * OL + ol (k < KS) takes output o = o0 + ol of the tile
//       o0 = 0, OL, 2 OL, ... and slice k: part_k = +0; part_k = part_k + v[i] * W[i][o] for i = k SL .. min((k + 1) SL, I) - 1 in order
//       (a slice past I is empty: +0).  Then out[o] = bias[o]; out[o] = out[o] + part_k for k = 0 .. KS - 1.  Lanes run along a row of W.
//   fct (a reduction ALONG the rows: dh from w2 [R][C], dm from w1 [C][R])   wave w of 16 takes the outputs o = w, w + 16, ...; lane l
//       adds v[i] * W[o][i] for i = l, l + 64, ... in order from +0; the 64 lane sums fold by the butterfly of fusegrad.hip (v = v + the v
//       of lane l ^ 32, then l ^ 16, 8, 4, 2, 1).
//
//   forward, 3 launches    se_sum_kernel (S slabs);  se_fc_forward_kernel (m = S / (float)N, z1 = fc(m, w1, b1), h = z1 * yr_sigmoid(z1),
//                          z2 = fc(h, w2, b2), g = yr_sigmoid(z2); writes m, z1, g);  se_scale_kernel (y = x * g[b][c]).
//   backward, <= 4 launches  se_dot_kernel (dg slabs);  se_fc_backward_kernel (dg from the slabs; t = 1.0f - g; u = g * t; dz2 = dg * u;
//                          h from z1 by the forward's operations; dh = fct(dz2, w2); dz1 = dh * tc_swish_grad(z1); with dx:
//                          dm = fct(dz1, w1), q = dm / (float)N; keeps dz2, h, dz1 [with parameters] and q [with dx] in the workspace);
//                          with parameters se_param_kernel (one lane an element of dw2, dw1, db2, db1: the batch's terms in increasing
//                          b, the first term image 0's own: db2[c] = sum_b dz2[b][c]; dw2[r][c] = sum_b h[b][r] * dz2[b][c];
//                          db1[r] = sum_b dz1[b][r]; dw1[c][r] = sum_b m[b][c] * dz1[b][r]);  with dx se_dx_kernel
//                          (dx = dy * g[b][c] + q[b][c]: a rounded product, then a rounded addition).
//                          3 launches with dx or the parameters alone, none with neither.
#include "train_common.h"

// The chunk.  A stage-1 workgroup should have SE_MIN_ELEMS = 4096 (pixel, channel) pairs of its block, 16 a lane, before its LDS fold and
// its slab pay off; an image is cut into at most SE_MAX_CHUNKS = 16 ranges, because every image's slabs are added by ONE workgroup of the
// small kernel that follows (16 loads a channel, all in flight).  At 64 images on the 256 CUs (2048 resident waves at 8 a SIMD):
//   13 x 13 x 512 (few pixels): Cb = 64, the minimum of 64 pixels sets the chunk, 169 pixels are 3 ranges: 8 blocks x 3 x 64 images =
//       1536 workgroups = 6144 waves, three full rounds of the machine; a minimum of 8192 pairs would leave ranges of 128 and 41 pixels;
//   52 x 52 x 128 (many pixels): the minimum would give 43 ranges, the cap gives 16 of 169 pixels: 2 blocks x 16 x 64 = 2048 workgroups =
//       8192 waves, four rounds, each lane 42 pixels deep; stage 2 reads 16 slabs an image instead of 43.
#define SE_THREADS 256         // lanes per workgroup of the map passes
#define SE_CB 64               // channels per workgroup, at most
#define SE_MIN_ELEMS 4096      // (pixel, channel) pairs per stage-1 workgroup, at least
#define SE_MAX_CHUNKS 16       // ranges (slabs) per image, at most
#define SE_FC_THREADS 1024     // lanes per workgroup of the small kernels: one workgroup an image
#define SE_MAX_C 4096          // the small kernels hold a [C] and an [R] vector in LDS: the contract's bounds (B7's widest block is
#define SE_MAX_R 1024          // C = 3840, R = 160)
#define SE_MAX_GRID (1 << 30)  // workgroups along x; more (image, range) pairs than that are walked with a grid stride

struct se_geo {
    long long N, chunk, units;      // pixels per image, pixels per range, B * nchunks
    int B, C, R, Cb, PP, nb, nchunks;
    float fn;                       // (float)N
};

static inline bool se_sizes_ok(int B, long long N, int C) {
    return B >= 1 && N >= 1 && C >= 1 && C <= SE_MAX_C && N < (1ll << 40) && (long long)B <= ((1ll << 40) - 1) / N;
}

static inline int se_cb(int C) {
    const int nb = (C + SE_CB - 1) / SE_CB;
    return (C + nb - 1) / nb;
}

static inline long long se_chunk(long long N, int C) { return tc_chunk(N, (SE_MIN_ELEMS + se_cb(C) - 1) / se_cb(C), SE_MAX_CHUNKS); }

static inline se_geo se_make_geo(int B, long long N, int C, int R) {
    se_geo g;
    g.N = N;
    g.chunk = se_chunk(N, C);
    g.B = B;
    g.C = C;
    g.R = R;
    g.nb = (C + SE_CB - 1) / SE_CB;
    g.Cb = se_cb(C);
    g.PP = SE_THREADS / g.Cb;
    g.nchunks = (int)((N + g.chunk - 1) / g.chunk);
    g.units = (long long)B * g.nchunks;
    g.fn = (float)N;
    return g;
}

// the chunk does not depend on B: an image alone and the same image inside a batch are summed in the same order
extern "C" long long yr_se_chunk(int B, long long N, int C) { return se_sizes_ok(B, N, C) ? se_chunk(N, C) : 0; }

// slabs [B][nchunks][C], then (the backward's) dz2 [B][C], q [B][C], h [B][R], dz1 [B][R]: one size for both calls
extern "C" size_t yr_se_workspace_bytes(int B, long long N, int C, int R) {
    if (!se_sizes_ok(B, N, C) || R < 1 || R > SE_MAX_R) return 0;
    const se_geo g = se_make_geo(B, N, C, R);
    return ((size_t)g.units * C + (size_t)2 * B * C + (size_t)2 * B * R) * sizeof(float);
}

struct se_ws {
    float *slabs, *dz2, *q, *h, *dz1;
};

static inline se_ws se_carve(void* workspace, const se_geo& g) {
    se_ws w;
    w.slabs = (float*)workspace;
    w.dz2 = w.slabs + (size_t)g.units * g.C;
    w.q = w.dz2 + (size_t)g.B * g.C;
    w.h = w.q + (size_t)g.B * g.C;
    w.dz1 = w.h + (size_t)g.B * g.R;
    return w;
}

// ---------------------------------------------------------------- the map passes
// what a lane of a map pass knows: its channel, whether it works, and (per unit) its first pixel and the end of the range as ROW numbers
// over the batch (b * N + p)
struct se_lane {
    int cl, po, c;
    bool on;
};

__device__ __forceinline__ se_lane se_lane_of(const se_geo& g) {
    se_lane l;
    l.po = (int)threadIdx.x / g.Cb;
    l.cl = (int)threadIdx.x - l.po * g.Cb;
    l.c = (int)blockIdx.y * g.Cb + l.cl;
    l.on = l.po < g.PP && l.c < g.C;
    return l;
}

// unit u = b * nchunks + j -> the image, and the rows [*r0, *r1) of the range
__device__ __forceinline__ long long se_range(const se_geo& g, long long u, long long* r0, long long* r1) {
    const long long b = u / g.nchunks;
    const long long p0 = (u - b * g.nchunks) * g.chunk;
    const long long p1 = p0 + g.chunk < g.N ? p0 + g.chunk : g.N;
    *r0 = b * g.N + p0;
    *r1 = b * g.N + p1;
    return b;
}

// the lanes' partial sums of one channel, added in the order of po from +0; lane po = 0 of the channel writes element c of slab u
__device__ __forceinline__ void se_fold(const se_geo& g, const se_lane& l, float acc, float* red, float* __restrict__ slabs, long long u) {
    red[threadIdx.x] = acc;
    __syncthreads();
    if (l.po == 0 && l.c < g.C) {
        const float* col = red + l.cl;
        float v = 0.0f;
        int k = 0;
        for (; k + 8 <= g.PP; k += 8) {      // (eight LDS reads in flight, then their additions in order)
            float r[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = col[(k + i) * g.Cb];
#pragma unroll
            for (int i = 0; i < 8; ++i) v = v + r[i];
        }
        for (; k < g.PP; ++k) v = v + col[k * g.Cb];
        slabs[(size_t)u * g.C + l.c] = v;
    }
    __syncthreads();      // red is written again by the next unit
}

// DOT: the slabs of sum_p a * b (dg); else of sum_p a (S; b is not read)
template <bool DOT>
__global__ __launch_bounds__(SE_THREADS) void se_sum_kernel(const float* __restrict__ a, long long a_ld, const float* __restrict__ b, long long b_ld,
                                                           se_geo g, float* __restrict__ slabs) {
    __shared__ float red[SE_THREADS];
    const se_lane l = se_lane_of(g);
    for (long long u = blockIdx.x; u < g.units; u += gridDim.x) {
        long long r0, r1;
        se_range(g, u, &r0, &r1);
        float acc = 0.0f;
        if (l.on) {
            const float* ap = a + l.c;
            const float* bp = DOT ? b + l.c : nullptr;
#pragma unroll 4
            for (long long r = r0 + l.po; r < r1; r += g.PP) {
                if (DOT) {
                    const float pr = ap[r * a_ld] * bp[r * b_ld];
                    acc = acc + pr;
                } else {
                    acc = acc + ap[r * a_ld];
                }
            }
        }
        se_fold(g, l, acc, red, slabs, u);
    }
}

// ADD: out = a * gate[b][c] + add[b][c] (dx); else out = a * gate[b][c] (y)
template <bool ADD>
__global__ __launch_bounds__(SE_THREADS) void se_scale_kernel(const float* __restrict__ a, long long a_ld, se_geo g, const float* __restrict__ gate,
                                                             const float* __restrict__ add, float* __restrict__ out, long long out_ld) {
    const se_lane l = se_lane_of(g);
    if (!l.on) return;
    for (long long u = blockIdx.x; u < g.units; u += gridDim.x) {
        long long r0, r1;
        const long long b = se_range(g, u, &r0, &r1);
        const float gv = gate[(size_t)b * g.C + l.c];
        const float qv = ADD ? add[(size_t)b * g.C + l.c] : 0.0f;
        const float* ap = a + l.c;
        float* op = out + l.c;
#pragma unroll 4
        for (long long r = r0 + l.po; r < r1; r += g.PP) {
            const float pr = ap[r * a_ld] * gv;
            op[r * out_ld] = ADD ? pr + qv : pr;
        }
    }
}

// ---------------------------------------------------------------- the small kernels
// stage 2 of a sum over the pixels: element c of image b's slabs, in index order from +0
__device__ __forceinline__ float se_slab_sum(const float* __restrict__ slabs, const se_geo& g, long long b, int c) {
    const float* sp = slabs + (size_t)b * g.nchunks * g.C + c;
    float r[SE_MAX_CHUNKS];
#pragma unroll
    for (int j = 0; j < SE_MAX_CHUNKS; ++j) r[j] = j < g.nchunks ? sp[(size_t)j * g.C] : 0.0f;
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < SE_MAX_CHUNKS; ++j)
        if (j < g.nchunks) v = v + r[j];
    return v;
}

// fc of the header: v [I] in LDS, W [I][O], bias [O]; done(o, value) once per output.  Every lane of the workgroup calls it.
template <class F>
__device__ __forceinline__ void se_fc(const float* v, int I, const float* __restrict__ W, int O, const float* __restrict__ bias, float* red, F done) {
    const int t = (int)threadIdx.x;
    const int OL = O < SE_FC_THREADS ? O : SE_FC_THREADS;
    const int KS = SE_FC_THREADS / OL;
    const int SL = (I + KS - 1) / KS;
    const int k = t / OL, ol = t - k * OL;
    for (int o0 = 0; o0 < O; o0 += OL) {
        const int o = o0 + ol;
        if (k < KS) {
            float acc = 0.0f;
            if (o < O) {
                const int i0 = k * SL;
                const int i1 = i0 + SL < I ? i0 + SL : I;
                const float* wp = W + o;
#pragma unroll 8
                for (int i = i0; i < i1; ++i) {
                    const float pr = v[i] * wp[(size_t)i * O];
                    acc = acc + pr;
                }
            }
            red[t] = acc;
        }
        __syncthreads();
        if (k == 0 && o < O) {
            float s = bias[o];
            for (int kk = 0; kk < KS; ++kk) s = s + red[kk * OL + ol];
            done(o, s);
        }
        __syncthreads();
    }
}

// fct of the header: v [I] in LDS, W [O][I]; done(o, value) once per output, by lane 0 of the output's wave
template <class F>
__device__ __forceinline__ void se_fct(const float* v, int I, const float* __restrict__ W, int O, F done) {
    const int w = (int)threadIdx.x >> 6, l = (int)threadIdx.x & 63;
    for (int o = w; o < O; o += SE_FC_THREADS / 64) {
        const float* wp = W + (size_t)o * I;
        float acc = 0.0f;
#pragma unroll 4
        for (int i = l; i < I; i += 64) {
            const float pr = v[i] * wp[i];
            acc = acc + pr;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
        if (l == 0) done(o, acc);
    }
}

__global__ __launch_bounds__(SE_FC_THREADS) void se_fc_forward_kernel(const float* __restrict__ slabs, se_geo g, const float* __restrict__ w1,
                                                                     const float* __restrict__ b1, const float* __restrict__ w2,
                                                                     const float* __restrict__ b2, float* __restrict__ m, float* __restrict__ z1,
                                                                     float* __restrict__ gate) {
    __shared__ float sv[SE_MAX_C];
    __shared__ float sh[SE_MAX_R];
    __shared__ float red[SE_FC_THREADS];
    for (long long b = blockIdx.x; b < g.B; b += gridDim.x) {
        for (int c = (int)threadIdx.x; c < g.C; c += SE_FC_THREADS) {
            const float mv = se_slab_sum(slabs, g, b, c) / g.fn;
            sv[c] = mv;
            m[(size_t)b * g.C + c] = mv;
        }
        __syncthreads();
        float* z1b = z1 + (size_t)b * g.R;
        se_fc(sv, g.C, w1, g.R, b1, red, [&](int r, float z) {
            z1b[r] = z;
            sh[r] = yr_apply_act(z, YR_ACT_SWISH);
        });
        float* gb = gate + (size_t)b * g.C;
        se_fc(sh, g.R, w2, g.C, b2, red, [&](int c, float z) { gb[c] = yr_sigmoid(z); });      // (se_fc ends on a barrier: sv and sh are free)
    }
}

__global__ __launch_bounds__(SE_FC_THREADS) void se_fc_backward_kernel(const float* __restrict__ slabs, se_geo g, const float* __restrict__ w1,
                                                                      const float* __restrict__ w2, const float* __restrict__ z1,
                                                                      const float* __restrict__ gate, bool params, bool want_dx,
                                                                      float* __restrict__ dz2, float* __restrict__ q, float* __restrict__ h,
                                                                      float* __restrict__ dz1) {
    __shared__ float sv[SE_MAX_C];
    __shared__ float sh[SE_MAX_R];
    for (long long b = blockIdx.x; b < g.B; b += gridDim.x) {
        for (int c = (int)threadIdx.x; c < g.C; c += SE_FC_THREADS) {
            const float dg = se_slab_sum(slabs, g, b, c);
            const float gv = gate[(size_t)b * g.C + c];
            const float t = 1.0f - gv;
            const float u = gv * t;
            const float d = dg * u;
            sv[c] = d;
            if (params) dz2[(size_t)b * g.C + c] = d;
        }
        const float* z1b = z1 + (size_t)b * g.R;
        if (params)
            for (int r = (int)threadIdx.x; r < g.R; r += SE_FC_THREADS) h[(size_t)b * g.R + r] = yr_apply_act(z1b[r], YR_ACT_SWISH);
        __syncthreads();
        float* dz1b = dz1 + (size_t)b * g.R;
        se_fct(sv, g.C, w2, g.R, [&](int r, float dh) {
            const float d = dh * tc_swish_grad(z1b[r]);
            sh[r] = d;
            if (params) dz1b[r] = d;
        });
        __syncthreads();
        if (want_dx) {
            float* qb = q + (size_t)b * g.C;
            se_fct(sh, g.R, w1, g.C, [&](int c, float dm) { qb[c] = dm / g.fn; });
        }
        __syncthreads();      // sv and sh are written again by the next image
    }
}

// one lane an element of dw2 [R][C], dw1 [C][R], db2 [C], db1 [R], in this order over the grid
__global__ __launch_bounds__(SE_THREADS) void se_param_kernel(se_geo g, const float* __restrict__ m, const float* __restrict__ dz2,
                                                             const float* __restrict__ h, const float* __restrict__ dz1, float* __restrict__ dw1,
                                                             float* __restrict__ db1, float* __restrict__ dw2, float* __restrict__ db2) {
    const int rc = g.R * g.C;
    int e = (int)blockIdx.x * SE_THREADS + (int)threadIdx.x;
    const float *ap = nullptr, *bp;
    long long a_ld = 0, b_ld;
    float* out;
    if (e < rc) {      // dw2[r][c] = sum_b h[b][r] * dz2[b][c]
        const int r = e / g.C, c = e - r * g.C;
        ap = h + r; a_ld = g.R; bp = dz2 + c; b_ld = g.C; out = dw2 + e;
    } else if (e < 2 * rc) {      // dw1[c][r] = sum_b m[b][c] * dz1[b][r]
        e -= rc;
        const int c = e / g.R, r = e - c * g.R;
        ap = m + c; a_ld = g.C; bp = dz1 + r; b_ld = g.R; out = dw1 + e;
    } else if (e < 2 * rc + g.C) {      // db2[c] = sum_b dz2[b][c]
        e -= 2 * rc;
        bp = dz2 + e; b_ld = g.C; out = db2 + e;
    } else if (e < 2 * rc + g.C + g.R) {      // db1[r] = sum_b dz1[b][r]
        e -= 2 * rc + g.C;
        bp = dz1 + e; b_ld = g.R; out = db1 + e;
    } else {
        return;
    }
    float v = ap ? ap[0] * bp[0] : bp[0];      // the first term image 0's own
#pragma unroll 4
    for (long long b = 1; b < g.B; ++b) {
        const float term = ap ? ap[b * a_ld] * bp[b * b_ld] : bp[b * b_ld];
        v = v + term;
    }
    *out = v;
}

// ---------------------------------------------------------------- entries
static inline dim3 se_map_grid(const se_geo& g) { return dim3((unsigned)(g.units < SE_MAX_GRID ? g.units : SE_MAX_GRID), (unsigned)g.nb); }
static inline dim3 se_fc_grid(const se_geo& g) { return dim3((unsigned)(g.B < SE_MAX_GRID ? g.B : SE_MAX_GRID)); }

// the checks the two entries share -> the geometry
static int se_check(const char* who, int B, int H, int W, int C, int R, const int* lds, int nld, void* workspace, size_t workspace_bytes, se_geo* g) {
    YR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && se_sizes_ok(B, (long long)H * W, C), "%s: B, H, W must be positive, B * H * W below 2^40 and C 1..%d (%d, %d, %d, %d)",
               who, SE_MAX_C, B, H, W, C);
    YR_REQUIRE(R >= 1 && R <= SE_MAX_R, "%s: R must be 1..%d, not %d", who, SE_MAX_R, R);
    const long long N = (long long)H * W;
    for (int i = 0; i < nld; ++i) {
        YR_REQUIRE(lds[i] >= C, "%s: a leading dimension below C = %d", who, C);
        YR_REQUIRE(tc_rows_fit((long long)B * N, lds[i]), "%s: byte offsets beyond 2^63", who);
    }
    const int rc = tc_workspace_check(who, workspace, workspace_bytes, yr_se_workspace_bytes(B, N, C, R));
    if (rc != YR_OK) return rc;
    *g = se_make_geo(B, N, C, R);
    return YR_OK;
}

extern "C" int yr_se_forward(const float* x, int x_ld, const float* w1, const float* b1, const float* w2, const float* b2, int B, int H, int W, int C,
                             int R, float* y, int y_ld, float* m, float* z1, float* gate, void* workspace, size_t workspace_bytes, void* stream) {
    YR_REQUIRE(x && w1 && b1 && w2 && b2 && y && m && z1 && gate, "se_forward: null pointer");
    YR_REQUIRE(((uintptr_t)x | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)b2 | (uintptr_t)y | (uintptr_t)m | (uintptr_t)z1 |
                (uintptr_t)gate) % 4 == 0, "se_forward: pointer not 4-byte aligned");
    se_geo g;
    const int lds[2] = {x_ld, y_ld};
    const int rc = se_check("se_forward", B, H, W, C, R, lds, 2, workspace, workspace_bytes, &g);
    if (rc != YR_OK) return rc;
    const se_ws ws = se_carve(workspace, g);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(se_sum_kernel<false>, se_map_grid(g), dim3(SE_THREADS), 0, s, x, (long long)x_ld, (const float*)nullptr, 0ll, g, ws.slabs);
    YR_LAUNCH_CHECK();
    hipLaunchKernelGGL(se_fc_forward_kernel, se_fc_grid(g), dim3(SE_FC_THREADS), 0, s, (const float*)ws.slabs, g, w1, b1, w2, b2, m, z1, gate);
    YR_LAUNCH_CHECK();
    hipLaunchKernelGGL(se_scale_kernel<false>, se_map_grid(g), dim3(SE_THREADS), 0, s, x, (long long)x_ld, g, (const float*)gate, (const float*)nullptr, y,
                       (long long)y_ld);
    YR_LAUNCH_CHECK();
    return YR_OK;
}

extern "C" int yr_se_backward(const float* dy, int dy_ld, const float* x, int x_ld, const float* w1, const float* w2, const float* m, const float* z1,
                              const float* gate, int B, int H, int W, int C, int R, float* dx, int dx_ld, float* dw1, float* db1, float* dw2, float* db2,
                              void* workspace, size_t workspace_bytes, void* stream) {
    YR_REQUIRE(dy && x && w1 && w2 && m && z1 && gate, "se_backward: null pointer");
    const bool params = dw1 != nullptr;
    YR_REQUIRE((db1 != nullptr) == params && (dw2 != nullptr) == params && (db2 != nullptr) == params,
               "se_backward: dw1, db1, dw2 and db2 go together: all or none");
    YR_REQUIRE(((uintptr_t)dy | (uintptr_t)x | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)m | (uintptr_t)z1 | (uintptr_t)gate | (uintptr_t)dx |
                (uintptr_t)dw1 | (uintptr_t)db1 | (uintptr_t)dw2 | (uintptr_t)db2) % 4 == 0, "se_backward: pointer not 4-byte aligned");
    se_geo g;
    const int lds[3] = {dy_ld, x_ld, dx ? dx_ld : C};
    const int rc = se_check("se_backward", B, H, W, C, R, lds, 3, workspace, workspace_bytes, &g);
    if (rc != YR_OK) return rc;
    if (!dx && !params) return YR_OK;      // nothing asked for: nothing launched
    const se_ws ws = se_carve(workspace, g);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(se_sum_kernel<true>, se_map_grid(g), dim3(SE_THREADS), 0, s, dy, (long long)dy_ld, x, (long long)x_ld, g, ws.slabs);
    YR_LAUNCH_CHECK();
    hipLaunchKernelGGL(se_fc_backward_kernel, se_fc_grid(g), dim3(SE_FC_THREADS), 0, s, (const float*)ws.slabs, g, w1, w2, z1, gate, params, dx != nullptr,
                       ws.dz2, ws.q, ws.h, ws.dz1);
    YR_LAUNCH_CHECK();
    if (params) {
        const long long n = 2ll * R * C + C + R;
        hipLaunchKernelGGL(se_param_kernel, dim3((unsigned)((n + SE_THREADS - 1) / SE_THREADS)), dim3(SE_THREADS), 0, s, g, m, (const float*)ws.dz2,
                           (const float*)ws.h, (const float*)ws.dz1, dw1, db1, dw2, db2);
        YR_LAUNCH_CHECK();
    }
    if (dx) {
        hipLaunchKernelGGL(se_scale_kernel<true>, se_map_grid(g), dim3(SE_THREADS), 0, s, dy, (long long)dy_ld, g, gate, (const float*)ws.q, dx,
                           (long long)dx_ld);
        YR_LAUNCH_CHECK();
    }
    return YR_OK;
}
