// Training of the output convolutions (the three *_y 1x1 convs of yolo3/model.py): the layer's forward on dense rows, the gradient
// of the loss with respect to its weights, and Keras Adam's dense update.  What the reference's _train_step (code/yolo3/train.py:18-46)
// does for these layers between the features and optimizer.apply_gradients, with the body frozen (code/train.py:150-171, "Train with
// frozen layers first"; ModelFactory.build carries the freeze commented out, so the frozen-body stage is build-defined).
//
// The conventions are those of train_common.h.  Rows: x [P][x_ld] (cin taken), dy / y [P][ld] (cout taken), P = B * H * W.  Weights
// are Wt[cout][kp], kp = round_up(cin, 4), the layout YR_OP_POINTWISE documents.  All products run on the float32 matrix pipe
// (the float16-plane split of the forward kernels is not used: a gradient summed over 10^5 pixels should not inherit a 2^-22
// operand cut).
//
// yr_linear_wgrad: dWt[co][ci] = sum_p dy[p][co] * x[p][ci].  Both operands load in their natural layout: for a quartet of pixels
// p0..p0+3, lane l holds A = dy[p0 + (l >> 4)][co0 + (l & 15)] and B = x[p0 + (l >> 4)][ci0 + (l & 15)] (A[i][k] with i the output
// channel and k the pixel, B[k][j] with j the input channel): sixteen lanes read 64 contiguous bytes of one row, no transpose.
// A lane past cin / cout in the last tile, or a pixel past the range in the last quartet, does not issue its load and contributes
// an exact zero.
//   stage 1  ht_wgrad_partial_kernel<TCO, TCI>: workgroup (c, bo, bi) owns pixels [c * chunk, (c + 1) * chunk) and TCO x TCI
//            tiles of 16 x 16.  Its 4 waves take chunk / 4 consecutive pixels each, keep all tiles in registers (5 x 5 tiles = 100
//            VGPRs: x and dy are read once at 75 x 75), then add their tiles in LDS in wave order and write one partial
//            [cout][kp] slab to the workspace.  cin or cout above 80: the tiles are blocked over the grid (operands re-read).
//   stage 2  yr_launch_slab_sum (tc_slab_sum_kernel, below; the depthwise weight gradient of convgrad.hip ends in it too): one lane
//            per element of dWt adds the slabs in index order and writes EVERY element, pad columns as +0.
// chunk depends on (pixels, cin, cout) only.
//
// yr_linear_forward: y[p][co] = sum_k x[p][k] * wt[co][k].  One wave per 16 pixels and up to 5 tiles of 16 output channels; lane l
// holds A = x[p0 + (l & 15)][4 s + (l >> 4)] and B = wt[co0 + (l & 15)][4 s + (l >> 4)] in step s.  Every y[p][0..cout) is written
// and nothing else.  Weight pad columns are not read.
//
// yr_adam_step: elementwise, in place, float32 in this order with nothing contracted (-ffp-contract=off):
//   m = b1 * m + (1 - b1) * g;  v = b2 * v + (1 - b2) * (g * g);  w = w - alpha * m / (sqrt(v) + eps)
// 1 - b1 and 1 - b2 are formed once in float32 (on the host, the same IEEE subtraction); sqrt and the division are the
// correctly rounded ones.  TF 2.x OptimizerV2 Adam without amsgrad, restated; tests/headtrain_ref.py is the definition.
#include "train_common.h"

#define HT_WAVES 4          // waves per workgroup of the gradient's stage 1
#define HT_U 2              // quartets of pixels a wave loads at a time
#define HT_MIN_CHUNK 256
#define HT_MAX_CHUNKS 2048

static inline bool ht_sizes_ok(long long pixels, int cin, int cout) {
    return pixels >= 1 && pixels < (1ll << 40) && cin >= 1 && cin <= 256 && cout >= 1 && cout <= 256;
}

// pixels per workgroup of stage 1: a multiple of 4 * HT_WAVES, so every wave starts on a quartet
// (the minimum is itself such a multiple, so rounding after the clamp is rounding before it)
static inline int ht_chunk(long long pixels, int cin, int cout) {
    const long long lo = (cin > 16 * TC_MAX_T || cout > 16 * TC_MAX_T) ? 2 * HT_MIN_CHUNK : HT_MIN_CHUNK;   // blocked tiles: larger slabs
    const long long c = tc_chunk(pixels, lo, HT_MAX_CHUNKS);
    return (int)((c + 4 * HT_WAVES - 1) / (4 * HT_WAVES) * (4 * HT_WAVES));
}

extern "C" int yr_linear_wgrad_chunk(long long pixels, int cin, int cout) {
    return ht_sizes_ok(pixels, cin, cout) ? ht_chunk(pixels, cin, cout) : 0;
}

extern "C" size_t yr_linear_wgrad_workspace_bytes(long long pixels, int cin, int cout) {
    if (!ht_sizes_ok(pixels, cin, cout)) return 0;
    const long long chunk = ht_chunk(pixels, cin, cout);
    return (size_t)((pixels + chunk - 1) / chunk) * (size_t)cout * (size_t)yr_round_up(cin, 4) * sizeof(float);
}

// ---------------------------------------------------------------- the weight gradient
template <int TCO, int TCI>
__global__ __launch_bounds__(64 * HT_WAVES, 3) void ht_wgrad_partial_kernel(const float* __restrict__ x, long long x_ld, const float* __restrict__ dy,
                                                                        long long dy_ld, long long pixels, int cin, int cout, int kp, int chunk,
                                                                        float* __restrict__ slabs) {
    __shared__ float red[TCO * TCI * 256];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int co0 = blockIdx.y * (TCO * 16), ci0 = blockIdx.z * (TCI * 16);
    const long long c0 = (long long)blockIdx.x * chunk;
    const long long c1 = c0 + chunk < pixels ? c0 + chunk : pixels;
    const int per = chunk / HT_WAVES;
    long long p = c0 + (long long)wave * per;
    const long long pend = p + per < c1 ? p + per : c1;      // (pend <= p: this wave has no pixels)

    bool aok[TCO], bok[TCI];
#pragma unroll
    for (int t = 0; t < TCO; ++t) aok[t] = co0 + 16 * t + l15 < cout;
#pragma unroll
    for (int t = 0; t < TCI; ++t) bok[t] = ci0 + 16 * t + l15 < cin;
    long long aoff = (p + g) * dy_ld + co0 + l15, boff = (p + g) * x_ld + ci0 + l15;      // element offsets of this lane's pixel row

    tc_f4 acc[TCO][TCI];
#pragma unroll
    for (int i = 0; i < TCO; ++i)
#pragma unroll
        for (int j = 0; j < TCI; ++j) acc[i][j] = (tc_f4){0.f, 0.f, 0.f, 0.f};

    float a[HT_U][TCO], b[HT_U][TCI];
    auto load = [&](float* av, float* bv, bool rowok, int q) {      // quartet q behind the current one
#pragma unroll
        for (int t = 0; t < TCO; ++t) av[t] = (rowok && aok[t]) ? dy[aoff + q * 4 * dy_ld + 16 * t] : 0.f;
#pragma unroll
        for (int t = 0; t < TCI; ++t) bv[t] = (rowok && bok[t]) ? x[boff + q * 4 * x_ld + 16 * t] : 0.f;
    };
    auto mac = [&](const float* av, const float* bv) {
#pragma unroll
        for (int i = 0; i < TCO; ++i)
#pragma unroll
            for (int j = 0; j < TCI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    };
    auto advance = [&](int quartets) { aoff += quartets * 4 * dy_ld; boff += quartets * 4 * x_ld; p += quartets * 4; };

    // groups of HT_U whole quartets, the next group's operands in flight while this group's products run; the quartets enter the
    // accumulators in pixel order whatever the grouping
    if (p + 4 * HT_U <= pend) {
#pragma unroll
        for (int u = 0; u < HT_U; ++u) load(a[u], b[u], true, u);
        while (p + 8 * HT_U <= pend) {
            float an[HT_U][TCO], bn[HT_U][TCI];
            advance(HT_U);
#pragma unroll
            for (int u = 0; u < HT_U; ++u) load(an[u], bn[u], true, u);
#pragma unroll
            for (int u = 0; u < HT_U; ++u) mac(a[u], b[u]);
#pragma unroll
            for (int u = 0; u < HT_U; ++u) {
#pragma unroll
                for (int t = 0; t < TCO; ++t) a[u][t] = an[u][t];
#pragma unroll
                for (int t = 0; t < TCI; ++t) b[u][t] = bn[u][t];
            }
        }
#pragma unroll
        for (int u = 0; u < HT_U; ++u) mac(a[u], b[u]);
        advance(HT_U);
    }
    while (p + 4 <= pend) {      // whole quartets short of a group (the end of the tensor)
        load(a[0], b[0], true, 0);
        mac(a[0], b[0]);
        advance(1);
    }
    if (p < pend) {      // the last, partial quartet of the pixel range (the end of the tensor)
        load(a[0], b[0], p + g < pend, 0);
        mac(a[0], b[0]);
    }

    // the waves' tiles, added in wave order
    for (int w = 0; w < HT_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < TCO; ++i)
#pragma unroll
                for (int j = 0; j < TCI; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int e = (i * TCI + j) * 256 + r * 64 + lane;
                        red[e] = w == 0 ? acc[i][j][r] : red[e] + acc[i][j][r];
                    }
        }
        __syncthreads();
    }
    float* slab = slabs + (size_t)blockIdx.x * ((size_t)cout * kp);
    for (int e = threadIdx.x; e < TCO * TCI * 256; e += 64 * HT_WAVES) {
        const int tile = e >> 8, r = (e >> 6) & 3, ln = e & 63;
        const int co = co0 + (tile / TCI) * 16 + (ln >> 4) * 4 + r;      // C/D map: column = lane & 15, row = (lane >> 4) * 4 + reg
        const int ci = ci0 + (tile % TCI) * 16 + (ln & 15);
        if (co < cout && ci < cin) slab[co * kp + ci] = red[e];
    }
}

// stage 2 of every two-stage sum of the training files (train_common.h): one lane per element.  (n is formed here, from the two
// factors: the compiler then gives the 32 loads of a round independent addresses; with n as an argument it chains them.)
__global__ __launch_bounds__(256) void tc_slab_sum_kernel(const float* __restrict__ slabs, int nchunks, int row_valid, int rows, int row_len,
                                                         float* __restrict__ out) {
    const int n = rows * row_len;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    if (e % row_len >= row_valid) { out[e] = 0.0f; return; }
    const float* s = slabs + e;
    float v = s[0];
#pragma unroll 32
    for (int c = 1; c < nchunks; ++c) v += s[(size_t)c * n];
    out[e] = v;
}

int yr_launch_slab_sum(const float* slabs, int nchunks, int rows, int row_len, int row_valid, float* out, hipStream_t s) {
    hipLaunchKernelGGL(tc_slab_sum_kernel, dim3((rows * row_len + 255) / 256), dim3(256), 0, s, slabs, nchunks, row_valid, rows, row_len, out);
    YR_LAUNCH_CHECK();
    return YR_OK;
}

template <int TCO>
static void ht_wgrad_launch_ci(int tci, dim3 grid, hipStream_t s, const float* x, long long x_ld, const float* dy, long long dy_ld,
                               long long pixels, int cin, int cout, int kp, int chunk, float* slabs) {
#define HT_CASE(T)                                                                                                          \
    case T:                                                                                                                 \
        hipLaunchKernelGGL((ht_wgrad_partial_kernel<TCO, T>), grid, dim3(64 * HT_WAVES), 0, s, x, x_ld, dy, dy_ld, pixels, cin, cout, kp, \
                           chunk, slabs);                                                                                   \
        break;
    switch (tci) { HT_CASE(1) HT_CASE(2) HT_CASE(3) HT_CASE(4) HT_CASE(5) }
#undef HT_CASE
}

extern "C" int yr_linear_wgrad(const float* x, int x_ld, const float* dy, int dy_ld, long long pixels, int cin, int cout,
                               void* workspace, size_t workspace_bytes, float* dwt, void* stream) {
    YR_REQUIRE(x && dy && workspace && dwt, "linear_wgrad: null pointer");
    YR_REQUIRE(ht_sizes_ok(pixels, cin, cout), "linear_wgrad: pixels must be 1..2^40-1 and cin, cout 1..256 (pixels %lld, cin %d, cout %d)", pixels, cin, cout);
    YR_REQUIRE(x_ld >= cin && dy_ld >= cout, "linear_wgrad: x_ld %d < cin %d or dy_ld %d < cout %d", x_ld, cin, dy_ld, cout);
    YR_REQUIRE(tc_rows_fit(pixels, x_ld) && tc_rows_fit(pixels, dy_ld), "linear_wgrad: byte offsets beyond 2^63");
    YR_REQUIRE(((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dwt) % 4 == 0, "linear_wgrad: x, dy or dwt not 4-byte aligned");
    const int rc = tc_workspace_check("linear_wgrad", workspace, workspace_bytes, yr_linear_wgrad_workspace_bytes(pixels, cin, cout));
    if (rc != YR_OK) return rc;
    const int kp = yr_round_up(cin, 4), chunk = ht_chunk(pixels, cin, cout);
    const int nchunks = (int)((pixels + chunk - 1) / chunk);
    int bo, to, bi, ti;
    tc_blocking(cout, &bo, &to);
    tc_blocking(cin, &bi, &ti);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(nchunks, bo, bi);
    float* slabs = (float*)workspace;
    switch (to) {
        case 1: ht_wgrad_launch_ci<1>(ti, grid, s, x, x_ld, dy, dy_ld, pixels, cin, cout, kp, chunk, slabs); break;
        case 2: ht_wgrad_launch_ci<2>(ti, grid, s, x, x_ld, dy, dy_ld, pixels, cin, cout, kp, chunk, slabs); break;
        case 3: ht_wgrad_launch_ci<3>(ti, grid, s, x, x_ld, dy, dy_ld, pixels, cin, cout, kp, chunk, slabs); break;
        case 4: ht_wgrad_launch_ci<4>(ti, grid, s, x, x_ld, dy, dy_ld, pixels, cin, cout, kp, chunk, slabs); break;
        default: ht_wgrad_launch_ci<5>(ti, grid, s, x, x_ld, dy, dy_ld, pixels, cin, cout, kp, chunk, slabs); break;
    }
    YR_LAUNCH_CHECK();
    return yr_launch_slab_sum(slabs, nchunks, cout, kp, cin, dwt, s);
}

// ---------------------------------------------------------------- the layer's forward
template <int NT>
__global__ __launch_bounds__(256) void ht_forward_kernel(const float* __restrict__ x, long long x_ld, const float* __restrict__ wt, long long pixels,
                                                        int cin, int cout, int kp, float* __restrict__ y, long long y_ld) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const long long p0 = ((long long)blockIdx.x * 4 + wave) * 16;
    if (p0 >= pixels) return;      // (wave-uniform)
    const int co0 = blockIdx.y * (NT * 16);
    const bool pok = p0 + l15 < pixels;
    const long long xoff = (p0 + l15) * x_ld;
    bool cok[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) cok[t] = co0 + 16 * t + l15 < cout;
    const int woff = (co0 + l15) * kp;
    tc_f4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (tc_f4){0.f, 0.f, 0.f, 0.f};
    for (int k = g; k < kp; k += 4) {      // kp is a multiple of 4: the same number of steps in every lane
        const bool kok = k < cin;
        const float a = (pok && kok) ? x[xoff + k] : 0.f;
        float b[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) b[t] = (cok[t] && kok) ? wt[woff + 16 * t * kp + k] : 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long p = p0 + g * 4 + r;      // C/D map: row = (lane >> 4) * 4 + reg (the pixel), column = lane & 15 (the channel)
        if (p < pixels) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (cok[t]) y[p * y_ld + co0 + 16 * t + l15] = acc[t][r];
        }
    }
}

extern "C" int yr_linear_forward(const float* x, int x_ld, const float* wt, long long pixels, int cin, int cout, float* y, int y_ld,
                                 void* stream) {
    YR_REQUIRE(x && wt && y, "linear_forward: null pointer");
    YR_REQUIRE(ht_sizes_ok(pixels, cin, cout), "linear_forward: pixels must be 1..2^40-1 and cin, cout 1..256 (pixels %lld, cin %d, cout %d)", pixels, cin, cout);
    YR_REQUIRE(x_ld >= cin && y_ld >= cout, "linear_forward: x_ld %d < cin %d or y_ld %d < cout %d", x_ld, cin, y_ld, cout);
    YR_REQUIRE(tc_rows_fit(pixels, x_ld) && tc_rows_fit(pixels, y_ld), "linear_forward: byte offsets beyond 2^63");
    YR_REQUIRE(((uintptr_t)x | (uintptr_t)wt | (uintptr_t)y) % 4 == 0, "linear_forward: x, wt or y not 4-byte aligned");
    const long long blocks = (pixels + 63) / 64;
    YR_REQUIRE(blocks <= INT_MAX, "linear_forward: more than 2^37 pixels");
    const int kp = yr_round_up(cin, 4);
    int bo, to;
    tc_blocking(cout, &bo, &to);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks, bo);
#define HT_CASE(T) \
    case T: hipLaunchKernelGGL(ht_forward_kernel<T>, grid, dim3(256), 0, s, x, (long long)x_ld, wt, pixels, cin, cout, kp, y, (long long)y_ld); break;
    switch (to) { HT_CASE(1) HT_CASE(2) HT_CASE(3) HT_CASE(4) HT_CASE(5) }
#undef HT_CASE
    YR_LAUNCH_CHECK();
    return YR_OK;
}

// ---------------------------------------------------------------- Adam
__global__ __launch_bounds__(256) void ht_adam_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                                                     long long n, float alpha, float beta1, float beta2, float omb1, float omb2, float eps) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float mi = beta1 * m[i] + omb1 * gi;
    const float vi = beta2 * v[i] + omb2 * (gi * gi);
    m[i] = mi;
    v[i] = vi;
    w[i] = w[i] - alpha * mi / (__builtin_sqrtf(vi) + eps);
}

extern "C" int yr_adam_step(float* w, float* m, float* v, const float* g, long long n, float alpha, float beta1, float beta2, float eps,
                            void* stream) {
    YR_REQUIRE(w && m && v && g, "adam_step: null pointer");
    YR_REQUIRE(n >= 1 && (n + 255) / 256 <= INT_MAX, "adam_step: n must be 1..2^39 (%lld)", n);
    YR_REQUIRE(((uintptr_t)w | (uintptr_t)m | (uintptr_t)v | (uintptr_t)g) % 4 == 0, "adam_step: pointer not 4-byte aligned");
    const float omb1 = 1.0f - beta1, omb2 = 1.0f - beta2;
    hipLaunchKernelGGL(ht_adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, m, v, g, n, alpha, beta1, beta2,
                       omb1, omb2, eps);
    YR_LAUNCH_CHECK();
    return YR_OK;
}
