// Backward operators of the layers behind the output convolutions (reference code/train.py:150-171 trains the whole neck and all
// heads): the input gradient of the bias-free 1x1 convolution, the k x k depthwise convolution on plain tensors with its two
// gradients, and the frozen BatchNorm + activation with its input gradient.  yoloret_amd/autograd.py wires them into torch.autograd;
// tests/convgrad_ref.py is the definition (the reference has no backward code of its own: TensorFlow's tape provides it).
//
// The conventions are those of train_common.h.
//
// yr_linear_dgrad: dx[p][ci] = sum_co dy[p][co] * wt[co][ci], wt = Wt[cout][kp] as yr_linear_forward reads it (pad columns not read).
//   On the float32 matrix pipe.  A workgroup of 4 waves owns 64 pixels and up to TC_MAX_T = 5 tiles of 16 input channels (tc_blocking);
//   each wave 16 pixels.  Wt is the B operand in its natural layout: lane l holds
//   wt[4 s + (l >> 4)][ci0 + (l & 15)], 64 contiguous bytes per sixteen lanes.  The A operand dy[p0 + (l & 15)][4 s + (l >> 4)] would be
//   a 16-byte gather per row straight from memory (the weakness of yr_linear_forward), so dy passes through LDS: per 64 output
//   channels a wave reads its 16 rows with 64 lanes along the row (256 contiguous bytes an instruction) into rows of 68 floats
//   (bank = 4 (l & 15) + (l >> 4) + const: no conflict), and takes A from there.  Channels past cout and pixels past the range are
//   stored as 0 and not loaded.  The 16 x 16 result (row = (l >> 4) * 4 + reg the pixel, column = l & 15 the channel) stores as 64-byte
//   row segments; dx[p][cin..dx_ld) is not touched.
//
// Depthwise maps are [B][H][W][ld] with C <= ld channels taken, taps w[k * k][C] (the Keras kernel [k, k, C, 1] reshaped), k in {3, 5},
// stride in {1, 2}; the padding is explicit: pad_top, pad_left (0..k-1) and the output size (OH, OW), which must be
// floor((H + pad_top + pad_bottom - k) / stride) + 1 for some pad_bottom in 0..k-1 (the same for columns): Keras 'same' and the
// explicit pad of MobileNetV2's stride-2 blocks both fit.  One lane per element at stride 2, per 4 consecutive columns of a channel at
// stride 1 (the window's columns and the weights are loaded once for the four), the channel the fastest index (lanes run along the
// row); the grid is (row of (column, channel) elements, map row, image), so no lane divides by more than C.
//   forward  y[b][oy][ox][c] = sum_t x[b][oy s - pt + ty][ox s - pl + tx][c] * w[t][c], taps in the order t = ty * k + tx, one fmaf each
//            from +0, out-of-range taps skipped.
//   dgrad    a gather: dx[b][iy][ix][c] = sum over the taps (ty, tx), in the same order, for which iy + pt - ty and ix + pl - tx are
//            multiples of the stride inside the output, of dy[b][.][.][c] * w[t][c].  At stride 2 only the taps of the matching parity
//            are visited: at most ceil(k / 2)^2.  Every dx[..][0..C) is written once.
//   wgrad    dw[t][c] = sum_{b, oy, ox} dy[b][oy][ox][c] * x[b][oy s - pt + ty][ox s - pl + tx][c] over in-range positions, two stages
//            like yr_linear_wgrad: stage 1, workgroup (chunk j, 64 channels): lane = channel, wave w of 8 takes the pixels w, w + 8, ... of
//            the chunk's output rows [j * chunk, (j + 1) * chunk) of the B * OH rows, k * k accumulators in registers; the waves' sums
//            are added in LDS in wave order and one [k * k][C] slab is written.  Stage 2 (yr_launch_slab_sum) adds the slabs in index
//            order and writes every dw element.  chunk = yr_depthwise_wgrad_chunk(B, OH, OW, C, k) rows.
//
// yr_bn_act_forward: u = z * scale[c] + shift[c] (a float32 multiply, then a float32 add), a = act(u) with act in {none, ReLU6, Swish}
// (yr_apply_act of yr_common.h); u is stored as well when asked for.  yr_bn_act_backward: dz = (da * act'(u)) * scale[c];
// act' as train_common.h states it; ReLU6: dz = +0 outside the open interval, whatever the scale.  scale and shift are frozen: no
// gradient for them.
#include "train_common.h"

#define CG_KC 64              // output channels per LDS pass
#define CG_LDS_LD 68          // floats per LDS row: 64 + 4, conflict-free for the A reads
#define CG_DW_NX 4             // output columns per lane of the stride-1 depthwise forward and input gradient
#define CG_DW_WAVES 8
#define CG_DW_MIN_PIXELS 128  // output pixels per workgroup of the depthwise weight gradient, at least
#define CG_DW_MAX_CHUNKS 1024

// ---------------------------------------------------------------- 1x1: the input gradient
template <int NT>
__global__ __launch_bounds__(256) void cg_dgrad_kernel(const float* __restrict__ dy, long long dy_ld, const float* __restrict__ wt, long long pixels,
                                                      int cin, int cout, int kp, float* __restrict__ dx, long long dx_ld) {
    __shared__ float tile[4][16 * CG_LDS_LD];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const long long p0 = ((long long)blockIdx.x * 4 + wave) * 16;      // (may lie past the range: such a wave loads and stores nothing)
    const int ci0 = blockIdx.y * (NT * 16);
    bool cok[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) cok[t] = ci0 + 16 * t + l15 < cin;
    tc_f4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (tc_f4){0.f, 0.f, 0.f, 0.f};
    float* mine = tile[wave];
    for (int c0 = 0; c0 < cout; c0 += CG_KC) {
        if (c0) __syncthreads();      // the previous pass has been read
        const bool colok = c0 + lane < cout;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long p = p0 + r;
            mine[r * CG_LDS_LD + lane] = (colok && p < pixels) ? dy[p * dy_ld + c0 + lane] : 0.f;
        }
        __syncthreads();
        const int steps = (cout - c0 < CG_KC ? cout - c0 + 3 : CG_KC) / 4;      // quartets of output channels in this pass
        for (int s = 0; s < steps; ++s) {
            const int co = c0 + 4 * s + g;
            const float a = mine[l15 * CG_LDS_LD + 4 * s + g];
            float b[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) b[t] = (cok[t] && co < cout) ? wt[co * kp + ci0 + 16 * t + l15] : 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long p = p0 + g * 4 + r;
        if (p < pixels) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (cok[t]) dx[p * dx_ld + ci0 + 16 * t + l15] = acc[t][r];
        }
    }
}

extern "C" int yr_linear_dgrad(const float* dy, int dy_ld, const float* wt, long long pixels, int cin, int cout, float* dx, int dx_ld,
                               void* stream) {
    YR_REQUIRE(dy && wt && dx, "linear_dgrad: null pointer");
    YR_REQUIRE(pixels >= 1 && pixels < (1ll << 40) && cin >= 1 && cin <= 256 && cout >= 1 && cout <= 256,
               "linear_dgrad: pixels must be 1..2^40-1 and cin, cout 1..256 (pixels %lld, cin %d, cout %d)", pixels, cin, cout);
    YR_REQUIRE(dy_ld >= cout && dx_ld >= cin, "linear_dgrad: dy_ld %d < cout %d or dx_ld %d < cin %d", dy_ld, cout, dx_ld, cin);
    YR_REQUIRE(tc_rows_fit(pixels, dy_ld) && tc_rows_fit(pixels, dx_ld), "linear_dgrad: byte offsets beyond 2^63");
    YR_REQUIRE(((uintptr_t)dy | (uintptr_t)wt | (uintptr_t)dx) % 4 == 0, "linear_dgrad: dy, wt or dx not 4-byte aligned");
    const long long blocks = (pixels + 63) / 64;
    YR_REQUIRE(blocks <= INT_MAX, "linear_dgrad: more than 2^37 pixels");
    const int kp = yr_round_up(cin, 4);
    int bi, ti;
    tc_blocking(cin, &bi, &ti);
    const dim3 grid((unsigned)blocks, bi);
    hipStream_t s = (hipStream_t)stream;
#define CG_CASE(T) \
    case T: hipLaunchKernelGGL(cg_dgrad_kernel<T>, grid, dim3(256), 0, s, dy, (long long)dy_ld, wt, pixels, cin, cout, kp, dx, (long long)dx_ld); break;
    switch (ti) { CG_CASE(1) CG_CASE(2) CG_CASE(3) CG_CASE(4) CG_CASE(5) }
#undef CG_CASE
    YR_LAUNCH_CHECK();
    return YR_OK;
}

// ---------------------------------------------------------------- depthwise
struct cg_dw {
    int B, H, W, C, OH, OW, pt, pl;
    long long x_ld, y_ld;      // leading dimensions of the input-side map (x / dx) and of the output-side map (y / dy)
};

// on = floor((n + pad + far - k) / stride) + 1 for some far pad in 0..k-1 (the smallest that gives on outputs)
static inline bool cg_dw_out_ok(int n, int on, int k, int stride, int pad) {
    long long far = (long long)(on - 1) * stride + k - pad - n;
    if (far < 0) far = 0;
    return far <= k - 1 && n + pad + far - k < (long long)on * stride;
}

static int cg_dw_check(const char* who, int B, int H, int W, int C, int k, int stride, int pt, int pl, int OH, int OW, int x_ld, int y_ld) {
    YR_REQUIRE(k == 3 || k == 5, "%s: k must be 3 or 5 (%d)", who, k);
    YR_REQUIRE(stride == 1 || stride == 2, "%s: stride must be 1 or 2 (%d)", who, stride);
    YR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1 && OH >= 1 && OW >= 1, "%s: B, H, W, C, OH, OW must be positive", who);
    YR_REQUIRE(B <= 65535 && H <= 65535 && OH <= 65535 && (long long)W * C < (1ll << 31) && (long long)OW * C < (1ll << 31),
               "%s: B, H, OH above 65535 or a row of 2^31 elements", who);
    YR_REQUIRE(pt >= 0 && pt < k && pl >= 0 && pl < k, "%s: pad_top %d / pad_left %d outside 0..k-1", who, pt, pl);
    YR_REQUIRE(x_ld >= C && y_ld >= C, "%s: a leading dimension below C = %d", who, C);
    YR_REQUIRE(cg_dw_out_ok(H, OH, k, stride, pt) && cg_dw_out_ok(W, OW, k, stride, pl),
               "%s: output %d x %d is not what input %d x %d, k %d, stride %d, pads (%d, %d) and a bottom / right pad in 0..k-1 give", who, OH, OW, H, W,
               k, stride, pt, pl);
    const long long in = (long long)B * H * W, out = (long long)B * OH * OW;
    YR_REQUIRE(in * x_ld < (1ll << 40) && out * y_ld < (1ll << 40) && in * C <= (long long)INT_MAX * 256 && out * C <= (long long)INT_MAX * 256,
               "%s: map too large", who);
    return YR_OK;
}

template <int K, int S>
__global__ __launch_bounds__(256) void cg_dw_forward_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, cg_dw d) {
    const unsigned e = blockIdx.x * 256u + threadIdx.x;      // (ox, c) of output row blockIdx.y of image blockIdx.z
    if (e >= (unsigned)(d.OW * d.C)) return;
    const int ox = (int)(e / (unsigned)d.C), c = (int)(e - (unsigned)ox * (unsigned)d.C);
    const int oy = blockIdx.y, b = blockIdx.z;
    const int iy0 = oy * S - d.pt, ix0 = ox * S - d.pl;
    float acc = 0.f;
#pragma unroll
    for (int ty = 0; ty < K; ++ty) {
        const int iy = iy0 + ty;
        if (iy < 0 || iy >= d.H) continue;
#pragma unroll
        for (int tx = 0; tx < K; ++tx) {
            const int ix = ix0 + tx;
            if (ix < 0 || ix >= d.W) continue;
            acc = __builtin_fmaf(x[(((long long)b * d.H + iy) * d.W + ix) * d.x_ld + c], w[(ty * K + tx) * d.C + c], acc);
        }
    }
    y[(((long long)b * d.OH + oy) * d.OW + ox) * d.y_ld + c] = acc;
}

template <int K, int S>
__global__ __launch_bounds__(256) void cg_dw_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx, cg_dw d) {
    const unsigned e = blockIdx.x * 256u + threadIdx.x;      // (ix, c) of input row blockIdx.y of image blockIdx.z
    if (e >= (unsigned)(d.W * d.C)) return;
    const int ix = (int)(e / (unsigned)d.C), c = (int)(e - (unsigned)ix * (unsigned)d.C);
    const int iy = blockIdx.y, b = blockIdx.z;
    const int ay = iy + d.pt, ax = ix + d.pl;      // ay - ty = oy * S
    float acc = 0.f;
#pragma unroll
    for (int jy = 0; jy < (K + S - 1) / S; ++jy) {
        const int ty = S == 1 ? jy : (ay & 1) + 2 * jy;
        const int ny = ay - ty;
        if (ty >= K || ny < 0 || ny / S >= d.OH) continue;
#pragma unroll
        for (int jx = 0; jx < (K + S - 1) / S; ++jx) {
            const int tx = S == 1 ? jx : (ax & 1) + 2 * jx;
            const int nx = ax - tx;
            if (tx >= K || nx < 0 || nx / S >= d.OW) continue;
            acc = __builtin_fmaf(dy[(((long long)b * d.OH + ny / S) * d.OW + nx / S) * d.y_ld + c], w[(ty * K + tx) * d.C + c], acc);
        }
    }
    dx[(((long long)b * d.H + iy) * d.W + ix) * d.x_ld + c] = acc;
}

// Stride 1: a lane owns CG_DW_NX consecutive columns of one channel.  Per tap row it loads the K + CG_DW_NX - 1 columns of the window
// once and each weight once (27 dword loads for 4 outputs at k = 3, where one column a lane takes 18 for one); every output still
// adds its taps in the order ty * k + tx, one fmaf each from +0, so the bits do not depend on the blocking.
template <int K>
__global__ __launch_bounds__(256) void cg_dw_forward_x4_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, cg_dw d) {
    const unsigned e = blockIdx.x * 256u + threadIdx.x;      // (column quartet, c) of output row blockIdx.y of image blockIdx.z
    const int nq = (d.OW + CG_DW_NX - 1) / CG_DW_NX;
    if (e >= (unsigned)(nq * d.C)) return;
    const int q = (int)(e / (unsigned)d.C), c = (int)(e - (unsigned)q * (unsigned)d.C);
    const int ox0 = q * CG_DW_NX, oy = blockIdx.y, b = blockIdx.z;
    const int ix0 = ox0 - d.pl;      // the window's first column
    float acc[CG_DW_NX];
#pragma unroll
    for (int o = 0; o < CG_DW_NX; ++o) acc[o] = 0.f;
#pragma unroll
    for (int ty = 0; ty < K; ++ty) {
        const int iy = oy - d.pt + ty;
        if (iy < 0 || iy >= d.H) continue;      // (the same for the whole workgroup)
        const float* row = x + (((long long)b * d.H + iy) * d.W) * d.x_ld + c;
        float xs[K + CG_DW_NX - 1];
        bool ok[K + CG_DW_NX - 1];
#pragma unroll
        for (int j = 0; j < K + CG_DW_NX - 1; ++j) {
            const int ix = ix0 + j;
            ok[j] = ix >= 0 && ix < d.W;
            xs[j] = ok[j] ? row[(long long)ix * d.x_ld] : 0.f;
        }
#pragma unroll
        for (int tx = 0; tx < K; ++tx) {
            const float wv = w[(ty * K + tx) * d.C + c];
#pragma unroll
            for (int o = 0; o < CG_DW_NX; ++o)
                if (ok[o + tx]) acc[o] = __builtin_fmaf(xs[o + tx], wv, acc[o]);
        }
    }
#pragma unroll
    for (int o = 0; o < CG_DW_NX; ++o)
        if (ox0 + o < d.OW) y[(((long long)b * d.OH + oy) * d.OW + ox0 + o) * d.y_ld + c] = acc[o];
}

template <int K>
__global__ __launch_bounds__(256) void cg_dw_dgrad_x4_kernel(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx, cg_dw d) {
    const unsigned e = blockIdx.x * 256u + threadIdx.x;      // (column quartet, c) of input row blockIdx.y of image blockIdx.z
    const int nq = (d.W + CG_DW_NX - 1) / CG_DW_NX;
    if (e >= (unsigned)(nq * d.C)) return;
    const int q = (int)(e / (unsigned)d.C), c = (int)(e - (unsigned)q * (unsigned)d.C);
    const int ix0 = q * CG_DW_NX, iy = blockIdx.y, b = blockIdx.z;
    const int nx0 = ix0 + d.pl - (K - 1);      // the window's first output column: tap tx of column ix0 + o reads window slot o - tx + K - 1
    float acc[CG_DW_NX];
#pragma unroll
    for (int o = 0; o < CG_DW_NX; ++o) acc[o] = 0.f;
#pragma unroll
    for (int ty = 0; ty < K; ++ty) {
        const int ny = iy + d.pt - ty;
        if (ny < 0 || ny >= d.OH) continue;      // (the same for the whole workgroup)
        const float* row = dy + (((long long)b * d.OH + ny) * d.OW) * d.y_ld + c;
        float ds[K + CG_DW_NX - 1];
        bool ok[K + CG_DW_NX - 1];
#pragma unroll
        for (int j = 0; j < K + CG_DW_NX - 1; ++j) {
            const int nx = nx0 + j;
            ok[j] = nx >= 0 && nx < d.OW;
            ds[j] = ok[j] ? row[(long long)nx * d.y_ld] : 0.f;
        }
#pragma unroll
        for (int tx = 0; tx < K; ++tx) {
            const float wv = w[(ty * K + tx) * d.C + c];
#pragma unroll
            for (int o = 0; o < CG_DW_NX; ++o)
                if (ok[o - tx + K - 1]) acc[o] = __builtin_fmaf(ds[o - tx + K - 1], wv, acc[o]);
        }
    }
#pragma unroll
    for (int o = 0; o < CG_DW_NX; ++o)
        if (ix0 + o < d.W) dx[(((long long)b * d.H + iy) * d.W + ix0 + o) * d.x_ld + c] = acc[o];
}

// output rows (of the B * OH) per workgroup of stage 1
static inline int cg_dw_chunk(int B, int OH, int OW) {
    return (int)tc_chunk((long long)B * OH, (CG_DW_MIN_PIXELS + OW - 1) / OW, CG_DW_MAX_CHUNKS);
}

static inline bool cg_dw_sizes_ok(int B, int OH, int OW, int C, int k) {
    return B >= 1 && OH >= 1 && OW >= 1 && C >= 1 && (k == 3 || k == 5) && (long long)B * OH * OW * C <= (long long)INT_MAX * 256;
}

extern "C" int yr_depthwise_wgrad_chunk(int B, int OH, int OW, int C, int k) { return cg_dw_sizes_ok(B, OH, OW, C, k) ? cg_dw_chunk(B, OH, OW) : 0; }

extern "C" size_t yr_depthwise_wgrad_workspace_bytes(int B, int OH, int OW, int C, int k) {
    if (!cg_dw_sizes_ok(B, OH, OW, C, k)) return 0;
    const long long chunk = cg_dw_chunk(B, OH, OW), rows = (long long)B * OH;
    return (size_t)((rows + chunk - 1) / chunk) * (size_t)(k * k) * (size_t)C * sizeof(float);
}

template <int K, int S>
__global__ __launch_bounds__(64 * CG_DW_WAVES) void cg_dw_wgrad_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                               float* __restrict__ slabs, cg_dw d, int chunk) {
    __shared__ float red[K * K * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.y * 64 + lane;
    const bool cok = c < d.C;
    const long long rows = (long long)d.B * d.OH;
    const long long r0 = (long long)blockIdx.x * chunk;
    const long long r1 = r0 + chunk < rows ? r0 + chunk : rows;
    const long long n = (r1 - r0) * d.OW;      // output pixels of this chunk
    float acc[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) acc[t] = 0.f;
    // this wave's pixels wave, wave + CG_DW_WAVES, ... of the chunk, walked as (image, row, column): no division in the loop
    int ox = wave % d.OW;
    long long row = r0 + wave / d.OW;
    int b = (int)(row / d.OH), oy = (int)(row % d.OH);
    for (long long i = wave; i < n; i += CG_DW_WAVES, ox += CG_DW_WAVES) {      // (wave-uniform)
        while (ox >= d.OW) {
            ox -= d.OW;
            ++row;
            if (++oy == d.OH) { oy = 0; ++b; }
        }
        const float g = cok ? dy[(row * d.OW + ox) * d.y_ld + c] : 0.f;
        const int iy0 = oy * S - d.pt, ix0 = ox * S - d.pl;
#pragma unroll
        for (int ty = 0; ty < K; ++ty) {
            const int iy = iy0 + ty;
            if (iy < 0 || iy >= d.H) continue;
#pragma unroll
            for (int tx = 0; tx < K; ++tx) {
                const int ix = ix0 + tx;
                if (ix < 0 || ix >= d.W) continue;
                const float xv = cok ? x[(((long long)b * d.H + iy) * d.W + ix) * d.x_ld + c] : 0.f;
                acc[ty * K + tx] = __builtin_fmaf(g, xv, acc[ty * K + tx]);
            }
        }
    }
    for (int wv = 0; wv < CG_DW_WAVES; ++wv) {      // the waves' sums, added in wave order
        if (wave == wv) {
#pragma unroll
            for (int t = 0; t < K * K; ++t) red[t * 64 + lane] = wv == 0 ? acc[t] : red[t * 64 + lane] + acc[t];
        }
        __syncthreads();
    }
    float* slab = slabs + (size_t)blockIdx.x * (size_t)(K * K) * d.C;
    for (int e = threadIdx.x; e < K * K * 64; e += 64 * CG_DW_WAVES) {
        const int cc = blockIdx.y * 64 + (e & 63);
        if (cc < d.C) slab[(e >> 6) * d.C + cc] = red[e];
    }
}

#define CG_DW_DISPATCH(KERNEL, grid, block, ...)                                                                  \
    do {                                                                                                          \
        if (k == 3 && stride == 1) hipLaunchKernelGGL((KERNEL<3, 1>), grid, block, 0, s, __VA_ARGS__);             \
        else if (k == 3) hipLaunchKernelGGL((KERNEL<3, 2>), grid, block, 0, s, __VA_ARGS__);                       \
        else if (stride == 1) hipLaunchKernelGGL((KERNEL<5, 1>), grid, block, 0, s, __VA_ARGS__);                  \
        else hipLaunchKernelGGL((KERNEL<5, 2>), grid, block, 0, s, __VA_ARGS__);                                   \
    } while (0)

extern "C" int yr_depthwise_forward(const float* x, int x_ld, const float* w, int B, int H, int W, int C, int k, int stride, int pad_top,
                                    int pad_left, int OH, int OW, float* y, int y_ld, void* stream) {
    YR_REQUIRE(x && w && y, "depthwise_forward: null pointer");
    YR_REQUIRE(((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) % 4 == 0, "depthwise_forward: x, w or y not 4-byte aligned");
    const int rc = cg_dw_check("depthwise_forward", B, H, W, C, k, stride, pad_top, pad_left, OH, OW, x_ld, y_ld);
    if (rc != YR_OK) return rc;
    const cg_dw d = {B, H, W, C, OH, OW, pad_top, pad_left, x_ld, y_ld};
    hipStream_t s = (hipStream_t)stream;
    if (stride == 1) {
        const dim3 grid((unsigned)(((long long)((OW + CG_DW_NX - 1) / CG_DW_NX) * C + 255) / 256), OH, B);
        if (k == 3) hipLaunchKernelGGL(cg_dw_forward_x4_kernel<3>, grid, dim3(256), 0, s, x, w, y, d);
        else hipLaunchKernelGGL(cg_dw_forward_x4_kernel<5>, grid, dim3(256), 0, s, x, w, y, d);
    } else {
        const dim3 grid((unsigned)(((long long)OW * C + 255) / 256), OH, B);
        if (k == 3) hipLaunchKernelGGL((cg_dw_forward_kernel<3, 2>), grid, dim3(256), 0, s, x, w, y, d);
        else hipLaunchKernelGGL((cg_dw_forward_kernel<5, 2>), grid, dim3(256), 0, s, x, w, y, d);
    }
    YR_LAUNCH_CHECK();
    return YR_OK;
}

extern "C" int yr_depthwise_dgrad(const float* dy, int dy_ld, const float* w, int B, int H, int W, int C, int k, int stride, int pad_top,
                                  int pad_left, int OH, int OW, float* dx, int dx_ld, void* stream) {
    YR_REQUIRE(dy && w && dx, "depthwise_dgrad: null pointer");
    YR_REQUIRE(((uintptr_t)dy | (uintptr_t)w | (uintptr_t)dx) % 4 == 0, "depthwise_dgrad: dy, w or dx not 4-byte aligned");
    const int rc = cg_dw_check("depthwise_dgrad", B, H, W, C, k, stride, pad_top, pad_left, OH, OW, dx_ld, dy_ld);
    if (rc != YR_OK) return rc;
    const cg_dw d = {B, H, W, C, OH, OW, pad_top, pad_left, dx_ld, dy_ld};
    hipStream_t s = (hipStream_t)stream;
    if (stride == 1) {
        const dim3 grid((unsigned)(((long long)((W + CG_DW_NX - 1) / CG_DW_NX) * C + 255) / 256), H, B);
        if (k == 3) hipLaunchKernelGGL(cg_dw_dgrad_x4_kernel<3>, grid, dim3(256), 0, s, dy, w, dx, d);
        else hipLaunchKernelGGL(cg_dw_dgrad_x4_kernel<5>, grid, dim3(256), 0, s, dy, w, dx, d);
    } else {
        const dim3 grid((unsigned)(((long long)W * C + 255) / 256), H, B);
        if (k == 3) hipLaunchKernelGGL((cg_dw_dgrad_kernel<3, 2>), grid, dim3(256), 0, s, dy, w, dx, d);
        else hipLaunchKernelGGL((cg_dw_dgrad_kernel<5, 2>), grid, dim3(256), 0, s, dy, w, dx, d);
    }
    YR_LAUNCH_CHECK();
    return YR_OK;
}

extern "C" int yr_depthwise_wgrad(const float* x, int x_ld, const float* dy, int dy_ld, int B, int H, int W, int C, int k, int stride,
                                  int pad_top, int pad_left, int OH, int OW, void* workspace, size_t workspace_bytes, float* dw, void* stream) {
    YR_REQUIRE(x && dy && workspace && dw, "depthwise_wgrad: null pointer");
    YR_REQUIRE(((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dw) % 4 == 0, "depthwise_wgrad: x, dy or dw not 4-byte aligned");
    const int rc = cg_dw_check("depthwise_wgrad", B, H, W, C, k, stride, pad_top, pad_left, OH, OW, x_ld, dy_ld);
    if (rc != YR_OK) return rc;
    const int wrc = tc_workspace_check("depthwise_wgrad", workspace, workspace_bytes, yr_depthwise_wgrad_workspace_bytes(B, OH, OW, C, k));
    if (wrc != YR_OK) return wrc;
    const int chunk = cg_dw_chunk(B, OH, OW);
    const int nchunks = (int)(((long long)B * OH + chunk - 1) / chunk);
    const cg_dw d = {B, H, W, C, OH, OW, pad_top, pad_left, x_ld, dy_ld};
    float* slabs = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    CG_DW_DISPATCH(cg_dw_wgrad_partial_kernel, dim3(nchunks, (C + 63) / 64), dim3(64 * CG_DW_WAVES), x, dy, slabs, d, chunk);
    YR_LAUNCH_CHECK();
    return yr_launch_slab_sum(slabs, nchunks, k * k, C, C, dw, s);
}

// ---------------------------------------------------------------- frozen BatchNorm + activation
__global__ __launch_bounds__(256) void cg_bn_act_forward_kernel(const float* __restrict__ z, long long z_ld, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, long long n, int C, int act, float* __restrict__ a,
                                                               long long a_ld, float* __restrict__ u, long long u_ld) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const long long p = e / C;
    const int c = (int)(e % C);
    const float m = z[p * z_ld + c] * scale[c];
    const float uv = m + shift[c];
    if (u) u[p * u_ld + c] = uv;
    a[p * a_ld + c] = yr_apply_act(uv, act);
}

__global__ __launch_bounds__(256) void cg_bn_act_backward_kernel(const float* __restrict__ da, long long da_ld, const float* __restrict__ u,
                                                                long long u_ld, const float* __restrict__ scale, long long n, int C, int act,
                                                                float* __restrict__ dz, long long dz_ld) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const long long p = e / C;
    const int c = (int)(e % C);
    const float g = da[p * da_ld + c], sc = scale[c];
    float r;
    if (act == YR_ACT_NONE) {
        r = g * sc;
    } else {
        const float uv = u[p * u_ld + c];
        if (act == YR_ACT_RELU6) r = tc_relu6_open(uv) ? g * sc : 0.0f;      // (the select around the product: +0 outside, whatever sc)
        else r = (g * tc_swish_grad(uv)) * sc;
    }
    dz[p * dz_ld + c] = r;
}

extern "C" int yr_bn_act_forward(const float* z, int z_ld, const float* scale, const float* shift, long long pixels, int C, int act, float* a,
                                 int a_ld, float* u, int u_ld, void* stream) {
    YR_REQUIRE(z && scale && shift && a, "bn_act_forward: null pointer");
    YR_REQUIRE(tc_act_ok(act), "bn_act_forward: act %d is not none, ReLU6 or Swish", act);
    YR_REQUIRE(pixels >= 1 && pixels < (1ll << 40) && C >= 1, "bn_act_forward: pixels must be 1..2^40-1 and C positive (pixels %lld, C %d)", pixels, C);
    YR_REQUIRE(z_ld >= C && a_ld >= C && (!u || u_ld >= C), "bn_act_forward: a leading dimension below C = %d", C);
    YR_REQUIRE(tc_rows_fit(pixels, z_ld) && tc_rows_fit(pixels, a_ld) && (!u || tc_rows_fit(pixels, u_ld)), "bn_act_forward: byte offsets beyond 2^63");
    YR_REQUIRE(((uintptr_t)z | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)a | (uintptr_t)u) % 4 == 0, "bn_act_forward: pointer not 4-byte aligned");
    const long long n = pixels * C;
    YR_REQUIRE((n + 255) / 256 <= INT_MAX, "bn_act_forward: more than 2^39 elements");
    hipLaunchKernelGGL(cg_bn_act_forward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, z, (long long)z_ld, scale, shift,
                       n, C, act, a, (long long)a_ld, u, (long long)u_ld);
    YR_LAUNCH_CHECK();
    return YR_OK;
}

extern "C" int yr_bn_act_backward(const float* da, int da_ld, const float* u, int u_ld, const float* scale, long long pixels, int C, int act,
                                  float* dz, int dz_ld, void* stream) {
    YR_REQUIRE(da && scale && dz && (u || act == YR_ACT_NONE), "bn_act_backward: null pointer");
    YR_REQUIRE(tc_act_ok(act), "bn_act_backward: act %d is not none, ReLU6 or Swish", act);
    YR_REQUIRE(pixels >= 1 && pixels < (1ll << 40) && C >= 1, "bn_act_backward: pixels must be 1..2^40-1 and C positive (pixels %lld, C %d)", pixels, C);
    YR_REQUIRE(da_ld >= C && dz_ld >= C && (!u || u_ld >= C), "bn_act_backward: a leading dimension below C = %d", C);
    YR_REQUIRE(tc_rows_fit(pixels, da_ld) && tc_rows_fit(pixels, dz_ld) && (!u || tc_rows_fit(pixels, u_ld)), "bn_act_backward: byte offsets beyond 2^63");
    YR_REQUIRE(((uintptr_t)da | (uintptr_t)u | (uintptr_t)scale | (uintptr_t)dz) % 4 == 0, "bn_act_backward: pointer not 4-byte aligned");
    const long long n = pixels * C;
    YR_REQUIRE((n + 255) / 256 <= INT_MAX, "bn_act_backward: more than 2^39 elements");
    hipLaunchKernelGGL(cg_bn_act_backward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, da, (long long)da_ld, u,
                       (long long)u_ld, scale, n, C, act, dz, (long long)dz_ld);
    YR_LAUNCH_CHECK();
    return YR_OK;
}
