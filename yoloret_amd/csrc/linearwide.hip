// The bias-free 1x1 convolution of any width up to 1024 channels on either side, with both gradients: what the neck and the heads of
// yolov3_body (code/yolo3/model.py:226-340: td1_conv 216..480 -> 512, td2_conv 424..576 -> 256, bu1_conv 331 -> 512, the 512 -> O
// projections) need to differentiate, and what yr_linear_forward / yr_linear_dgrad / yr_linear_wgrad (headtrain.hip, convgrad.hip;
// cin, cout <= 256, five tiles a workgroup) would only compute with the activations re-read once per 80 channels.  The entries
// accept the narrow widths too and give the narrow entries' bytes there (why: below).
//
// The conventions are those of train_common.h.  Rows: x / dx [P][ld] (cin taken), y / dy [P][ld] (cout taken), P = B * H * W.
// Weights are Wt[cout][kp], kp = round_up(cin, 4); pad columns are never read.
//
// yr_linear_wide_forward: y[p][co] = sum_k x[p][k] * wt[co][k];  yr_linear_wide_dgrad: dx[p][ci] = sum_co dy[p][co] * wt[co][ci].
//   One kernel, lw_product_kernel<WT, NAT>: out[p][n] = sum_k act[p][k] * W(k, n), with W(k, n) = wt[n][k] for the forward (NAT = false:
//   lane l holds wt[n0 + (l & 15)][4 s + (l >> 4)], 16-byte pieces of 16 rows, from the caches: the weights are small) and
//   W(k, n) = wt[k][n] for the input gradient (NAT = true, the natural layout: 64 contiguous bytes per sixteen lanes).
//   A workgroup of 4 waves owns 64 pixels and `per` <= 16 tiles of 16 output channels: 256 channels a pass over the activations, so a
//   256-wide output reads them once and a 512-wide one twice (tiles = ceil(n / 16), blocks = ceil(tiles / 16),
//   per = ceil(tiles / blocks)).  Wave w takes the WT = ceil(per / 4) <= 4 consecutive tiles w WT, w WT + 1, ... < per of the block (a
//   run of up to 256 contiguous bytes of every output row) for ALL 64 pixels: 4 x WT accumulators, 64 registers at WT = 4, and the
//   weights are read once per 64 pixels, not once per 16.  A tile at or past `per`, or wholly past the channel count, loads nothing,
//   multiplies nothing and stores nothing (a wave-uniform count of live tiles guards it); a wave without any tile only stages.  The activations pass through LDS, 64 channels at a time: wave w reads rows 16 w .. 16 w + 15 with its 64 lanes
//   along the row (256 contiguous bytes an instruction) into rows of 66 floats, the next pass's 16 registers in flight while this
//   pass's products run.  A = tile[16 i + (l & 15)][4 s + (l >> 4)] is a ds_read_b32 whose banks within a half-wave are
//   (2 (l & 15) + (l >> 4) + const) mod 32, all different: no conflict.  Channels past K and pixels past the range are staged as 0 and
//   not loaded.  The 16 x 16 result (row = (l >> 4) * 4 + reg the pixel, column = l & 15 the channel) stores as 64-byte row segments;
//   out[p][n..ld) is not touched.
//   Summation order: every output element is ONE accumulator; its products enter in the order k = 0, 1, 2, ... (MFMA steps of four,
//   k ascending inside a step), whatever the blocking.  That is the order of yr_linear_forward and yr_linear_dgrad: at widths both
//   accept the bytes are the same.
//
// yr_linear_wide_wgrad: dWt[co][ci] = sum_p dy[p][co] * x[p][ci], two stages like yr_linear_wgrad, operands in their natural layout
// (for a quartet of pixels lane l holds A = dy[p0 + (l >> 4)][co0 + (l & 15)] and B = x[p0 + (l >> 4)][ci0 + (l & 15)]).
//   stage 1  lw_wgrad_partial_kernel<TA, TB>: workgroup (c, bo, bi) owns pixels [c * chunk, (c + 1) * chunk) and per_co x per_ci <= 8 x 8
//            tiles of 16 x 16 (128 x 128 channels: x is read ceil(cout / 128) times and dy ceil(cin / 128) times, where the narrow
//            blocking reads them ceil(cout / 80) and ceil(cin / 80) times).  Both operands pass through LDS, 16 pixels a step: wave w
//            reads rows 4 w .. 4 w + 3 with its lanes along the row (256 contiguous bytes an instruction, each element once per
//            workgroup) into rows of 144 floats, the next step's 16 registers in flight while this step's products run; the operand
//            reads are ds_read_b32 whose banks within a half-wave are (16 (l >> 4) + (l & 15) + const) mod 32, all different.  The 4
//            waves split the TILES 2 x 2, not the pixels: wave (wa, wb) takes the TA = ceil(per_co / 2) <= 4 consecutive output-channel
//            tiles wa TA, wa TA + 1, ... < per_co and the input-channel tiles wb TB, ... < per_ci (TB likewise), 16 accumulators at
//            most, walks the whole chunk in pixel order and writes its tiles to the chunk's [cout][kp] slab: no sum across waves.  A
//            tile past per_* or wholly past the channel count is not loaded, not multiplied and not stored; channels past the count
//            and pixels past the range are staged as 0 and not loaded.
//   stage 2  yr_launch_slab_sum adds the slabs in index order and writes EVERY element of dWt, pad columns as +0.
//   Summation order: within a chunk one accumulator per element, quartets of pixels in ascending order (pixels ascending inside a
//   quartet); then the chunks in index order, the first term chunk 0's sum itself.
//   The chunk rule, yr_linear_wide_wgrad_chunk: the least multiple of 16 that is at least
//       LW_MIN_CHUNK = 64,   ceil(cout * kp / (cin + cout)),   ceil(pixels / LW_MAX_CHUNKS = 1024):
//   the second term makes one slab (cout * kp floats, written once and read once) no larger than the operands of its chunk
//   (chunk * (cin + cout) floats), the third keeps the slabs at 1024 (and the chunk of 2^40 - 1 pixels an int).  A function of the three sizes only.
//   Where cin AND cout are at most 256 the entry IS yr_linear_wgrad (headtrain.hip): its chunk (yr_linear_wgrad_chunk), its workspace,
//   its stage 1, which splits the PIXELS over the waves, its order and its bytes.  At a shape that is one 128 x 128 block the tile
//   split leaves nothing to gain (no operand is re-read either way) and measured 1.07 .. 1.21 of the narrow form's time at the
//   neck's 75 -> 128 and 248 -> 128 layers.  So stage 1 above runs only with a side above 256, where TA or TB is 3 or 4: the four
//   forms with both at most 2 do not exist.
#include "train_common.h"

#define LW_MAX_C 1024       // channels on either side
#define LW_PIX 64           // pixels per workgroup of the product kernel
#define LW_KC 64            // activation channels per LDS pass
#define LW_LDS_LD 66        // floats per LDS row: conflict-free for the A reads (above)
#define LW_WG_TILES 16      // 16-wide output tiles per workgroup of the product kernel, 4 per wave
#define LW_GW_TILES 8       // tiles per side and workgroup of the gradient's stage 1, 4 per wave
#define LW_GP 16            // pixels per LDS step of the gradient's stage 1
#define LW_GLD 144          // floats per LDS row there: 128 + 16, conflict-free for the operand reads (below)
#define LW_MIN_CHUNK 64
#define LW_MAX_CHUNKS 1024
#define LW_CHUNK_STEP 16

static inline bool lw_sizes_ok(long long pixels, int cin, int cout) {
    return pixels >= 1 && pixels < (1ll << 40) && cin >= 1 && cin <= LW_MAX_C && cout >= 1 && cout <= LW_MAX_C;
}

// n channels = tiles of 16 -> (blocks over the grid, tiles per block <= most)
static inline void lw_blocking(int n, int most, int* blocks, int* per) {
    const int t = (n + 15) / 16;
    *blocks = (t + most - 1) / most;
    *per = (t + *blocks - 1) / *blocks;
}

static inline int lw_chunk(long long pixels, int cin, int cout) {
    const long long kp = yr_round_up(cin, 4);
    long long c = tc_chunk(pixels, LW_MIN_CHUNK, LW_MAX_CHUNKS);
    const long long even = (cout * kp + cin + cout - 1) / (cin + cout);      // slab <= the chunk's operands
    if (c < even) c = even;
    return (int)((c + LW_CHUNK_STEP - 1) / LW_CHUNK_STEP * LW_CHUNK_STEP);
}

// both sides within the narrow entries' range: the weight gradient is theirs
static inline bool lw_narrow(int cin, int cout) { return cin <= 256 && cout <= 256; }

extern "C" int yr_linear_wide_wgrad_chunk(long long pixels, int cin, int cout) {
    if (!lw_sizes_ok(pixels, cin, cout)) return 0;
    return lw_narrow(cin, cout) ? yr_linear_wgrad_chunk(pixels, cin, cout) : lw_chunk(pixels, cin, cout);
}

extern "C" size_t yr_linear_wide_wgrad_workspace_bytes(long long pixels, int cin, int cout) {
    if (!lw_sizes_ok(pixels, cin, cout)) return 0;
    if (lw_narrow(cin, cout)) return yr_linear_wgrad_workspace_bytes(pixels, cin, cout);
    const long long chunk = lw_chunk(pixels, cin, cout);
    return (size_t)((pixels + chunk - 1) / chunk) * (size_t)cout * (size_t)yr_round_up(cin, 4) * sizeof(float);
}

// ---------------------------------------------------------------- the forward and the input gradient
template <int WT, bool NAT>
__global__ __launch_bounds__(256) void lw_product_kernel(const float* __restrict__ act, long long act_ld, const float* __restrict__ wt, long long pixels,
                                                        int K, int N, int kp, int per, float* __restrict__ out, long long out_ld) {
    __shared__ float tile[LW_PIX * LW_LDS_LD];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const long long p0 = (long long)blockIdx.x * LW_PIX;
    const int t0 = blockIdx.y * per;      // the block's first tile
    int n[WT];
    bool nok[WT];
#pragma unroll
    for (int j = 0; j < WT; ++j) {
        n[j] = (t0 + wave * WT + j) * 16 + l15;
        nok[j] = wave * WT + j < per && n[j] < N;
    }
    // (wave-uniform) the tiles of this wave that lie inside the block and begin inside the channel count: its first `live`
    int live = per - wave * WT;
    const int left = (N + 15) / 16 - (t0 + wave * WT);
    live = live < left ? live : left;
    live = live < WT ? live : WT;
    const bool any = live > 0;
    tc_f4 acc[4][WT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) acc[i][j] = (tc_f4){0.f, 0.f, 0.f, 0.f};

    // this wave's 16 rows of a pass, lanes along the row
    const long long prow = p0 + 16 * wave;
    float st[16];
    auto fetch = [&](int c0) {
        const bool colok = c0 + lane < K;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = (colok && prow + r < pixels) ? act[(prow + r) * act_ld + c0 + lane] : 0.f;
    };
    fetch(0);
    for (int c0 = 0; c0 < K; c0 += LW_KC) {
        if (c0) __syncthreads();      // the previous pass has been read
#pragma unroll
        for (int r = 0; r < 16; ++r) tile[(16 * wave + r) * LW_LDS_LD + lane] = st[r];
        __syncthreads();
        if (c0 + LW_KC < K) fetch(c0 + LW_KC);
        if (!any) continue;
        const int steps = (K - c0 < LW_KC ? K - c0 + 3 : LW_KC) / 4;      // quartets of channels in this pass
#pragma unroll 2
        for (int s = 0; s < steps; ++s) {
            const int k = c0 + 4 * s + g;
            const bool kok = k < K;
            float a[4], b[WT];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = tile[(16 * i + l15) * LW_LDS_LD + 4 * s + g];
#pragma unroll
            for (int j = 0; j < WT; ++j)
                if (j < live) b[j] = (nok[j] && kok) ? (NAT ? wt[k * kp + n[j]] : wt[n[j] * kp + k]) : 0.f;
#pragma unroll
            for (int j = 0; j < WT; ++j)
                if (j < live) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
                }
        }
    }
    if (!any) return;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = p0 + 16 * i + g * 4 + r;      // C/D map: row = (lane >> 4) * 4 + reg (the pixel), column = lane & 15 (the channel)
            if (p < pixels) {
#pragma unroll
                for (int j = 0; j < WT; ++j)
                    if (nok[j]) out[p * out_ld + n[j]] = acc[i][j][r];
            }
        }
}

// out [pixels][N] = act [pixels][K] * W: the launch of both entries (the caller has checked the sizes)
template <bool NAT>
static int lw_product_launch(const char* who, const float* act, int act_ld, const float* wt, long long pixels, int K, int N, int kp, float* out,
                             int out_ld, hipStream_t s) {
    const long long rows = (pixels + LW_PIX - 1) / LW_PIX;
    YR_REQUIRE(rows <= INT_MAX, "%s: more than 2^37 pixels", who);
    int blocks, per;
    lw_blocking(N, LW_WG_TILES, &blocks, &per);
    const dim3 grid((unsigned)rows, blocks);
#define LW_CASE(T)                                                                                                                      \
    case T:                                                                                                                             \
        return YR_LAUNCH((lw_product_kernel<T, NAT>), grid, dim3(256), 0, 0, s, ("lw_product_kernel<%d,%d>", T, (int)NAT), act, (long long)act_ld, wt, \
                         pixels, K, N, kp, per, out, (long long)out_ld);
    switch ((per + 3) / 4) { LW_CASE(1) LW_CASE(2) LW_CASE(3) LW_CASE(4) }
#undef LW_CASE
    return YR_ERR_ARG;      // (not reached: per is 1..16)
}

extern "C" int yr_linear_wide_forward(const float* x, int x_ld, const float* wt, long long pixels, int cin, int cout, float* y, int y_ld,
                                      void* stream) {
    YR_REQUIRE(x && wt && y, "linear_wide_forward: null pointer");
    YR_REQUIRE(lw_sizes_ok(pixels, cin, cout), "linear_wide_forward: pixels must be 1..2^40-1 and cin, cout 1..1024 (pixels %lld, cin %d, cout %d)", pixels, cin, cout);
    YR_REQUIRE(x_ld >= cin && y_ld >= cout, "linear_wide_forward: x_ld %d < cin %d or y_ld %d < cout %d", x_ld, cin, y_ld, cout);
    YR_REQUIRE(tc_rows_fit(pixels, x_ld) && tc_rows_fit(pixels, y_ld), "linear_wide_forward: byte offsets beyond 2^63");
    YR_REQUIRE(((uintptr_t)x | (uintptr_t)wt | (uintptr_t)y) % 4 == 0, "linear_wide_forward: x, wt or y not 4-byte aligned");
    return lw_product_launch<false>("linear_wide_forward", x, x_ld, wt, pixels, cin, cout, yr_round_up(cin, 4), y, y_ld, (hipStream_t)stream);
}

extern "C" int yr_linear_wide_dgrad(const float* dy, int dy_ld, const float* wt, long long pixels, int cin, int cout, float* dx, int dx_ld,
                                    void* stream) {
    YR_REQUIRE(dy && wt && dx, "linear_wide_dgrad: null pointer");
    YR_REQUIRE(lw_sizes_ok(pixels, cin, cout), "linear_wide_dgrad: pixels must be 1..2^40-1 and cin, cout 1..1024 (pixels %lld, cin %d, cout %d)", pixels, cin, cout);
    YR_REQUIRE(dy_ld >= cout && dx_ld >= cin, "linear_wide_dgrad: dy_ld %d < cout %d or dx_ld %d < cin %d", dy_ld, cout, dx_ld, cin);
    YR_REQUIRE(tc_rows_fit(pixels, dy_ld) && tc_rows_fit(pixels, dx_ld), "linear_wide_dgrad: byte offsets beyond 2^63");
    YR_REQUIRE(((uintptr_t)dy | (uintptr_t)wt | (uintptr_t)dx) % 4 == 0, "linear_wide_dgrad: dy, wt or dx not 4-byte aligned");
    return lw_product_launch<true>("linear_wide_dgrad", dy, dy_ld, wt, pixels, cout, cin, yr_round_up(cin, 4), dx, dx_ld, (hipStream_t)stream);
}

// ---------------------------------------------------------------- the weight gradient
template <int TA, int TB>
__global__ __launch_bounds__(256) void lw_wgrad_partial_kernel(const float* __restrict__ x, long long x_ld, const float* __restrict__ dy, long long dy_ld,
                                                              long long pixels, int cin, int cout, int kp, int chunk, int per_co, int per_ci,
                                                              float* __restrict__ slabs) {
    __shared__ float sa[LW_GP * LW_GLD], sb[LW_GP * LW_GLD];      // dy and x of LW_GP pixels, the block's channels
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int wa = wave & 1, wb = wave >> 1;
    const int ta0 = blockIdx.y * per_co + wa * TA, tb0 = blockIdx.z * per_ci + wb * TB;      // this wave's first tiles
    // (wave-uniform) the tiles of this wave that lie inside the block and begin inside the channel count: its first na x nb
    int na = per_co - wa * TA, nb = per_ci - wb * TB;
    const int lefta = (cout + 15) / 16 - ta0, leftb = (cin + 15) / 16 - tb0;
    na = na < lefta ? na : lefta;
    nb = nb < leftb ? nb : leftb;
    na = na < TA ? na : TA;
    nb = nb < TB ? nb : TB;
    const bool any = na > 0 && nb > 0;      // (a wave without a tile only stages)
    const long long c0 = (long long)blockIdx.x * chunk;
    const long long pend = c0 + chunk < pixels ? c0 + chunk : pixels;

    tc_f4 acc[TA][TB];
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
        for (int j = 0; j < TB; ++j) acc[i][j] = (tc_f4){0.f, 0.f, 0.f, 0.f};

    // staging: wave w brings rows 4 w .. 4 w + 3 of a step, its lanes along the row: channels lane and lane + 64 of the block on either
    // side (256 contiguous bytes an instruction); channels past the block or the count and pixels past the range are 0 and not loaded
    const int ca0 = blockIdx.y * per_co * 16, cb0 = blockIdx.z * per_ci * 16;      // the block's first channels
    bool sok[4];
    sok[0] = lane < per_co * 16 && ca0 + lane < cout;
    sok[1] = lane + 64 < per_co * 16 && ca0 + lane + 64 < cout;
    sok[2] = lane < per_ci * 16 && cb0 + lane < cin;
    sok[3] = lane + 64 < per_ci * 16 && cb0 + lane + 64 < cin;
    float st[4][4];
    auto fetch = [&](long long p0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = p0 + 4 * wave + r;
            const bool rowok = p < pend;
            st[r][0] = (rowok && sok[0]) ? dy[p * dy_ld + ca0 + lane] : 0.f;
            st[r][1] = (rowok && sok[1]) ? dy[p * dy_ld + ca0 + lane + 64] : 0.f;
            st[r][2] = (rowok && sok[2]) ? x[p * x_ld + cb0 + lane] : 0.f;
            st[r][3] = (rowok && sok[3]) ? x[p * x_ld + cb0 + lane + 64] : 0.f;
        }
    };
    fetch(c0);
    for (long long p0 = c0; p0 < pend; p0 += LW_GP) {
        if (p0 != c0) __syncthreads();      // the previous step has been read
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* ra = sa + (4 * wave + r) * LW_GLD + lane;
            float* rb = sb + (4 * wave + r) * LW_GLD + lane;
            ra[0] = st[r][0];
            ra[64] = st[r][1];
            rb[0] = st[r][2];
            rb[64] = st[r][3];
        }
        __syncthreads();
        if (p0 + LW_GP < pend) fetch(p0 + LW_GP);      // the next step's rows in flight while this step's products run
        if (!any) continue;
        // the step's quartets in pixel order; lane l holds A = dy[4 q + (l >> 4)][tile + (l & 15)] and B = x[..] likewise
#pragma unroll
        for (int q = 0; q < LW_GP / 4; ++q) {
            if (p0 + 4 * q >= pend) break;      // (uniform: whole quartets past the range)
            float a[TA], b[TB];
#pragma unroll
            for (int i = 0; i < TA; ++i)
                if (i < na) a[i] = sa[(4 * q + g) * LW_GLD + (wa * TA + i) * 16 + l15];
#pragma unroll
            for (int j = 0; j < TB; ++j)
                if (j < nb) b[j] = sb[(4 * q + g) * LW_GLD + (wb * TB + j) * 16 + l15];
#pragma unroll
            for (int i = 0; i < TA; ++i)
#pragma unroll
                for (int j = 0; j < TB; ++j)
                    if (i < na && j < nb) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    if (!any) return;

    float* slab = slabs + (size_t)blockIdx.x * ((size_t)cout * kp);
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            if (i >= na || j >= nb) continue;      // (wave-uniform)
            const int ci = (tb0 + j) * 16 + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = (ta0 + i) * 16 + g * 4 + r;      // C/D map: row = (lane >> 4) * 4 + reg, column = lane & 15
                if (co < cout && ci < cin) slab[co * kp + ci] = acc[i][j][r];
            }
        }
}

template <int TA>
static int lw_wgrad_launch_ci(int tb, dim3 grid, hipStream_t s, const float* x, long long x_ld, const float* dy, long long dy_ld, long long pixels,
                              int cin, int cout, int kp, int chunk, int per_co, int per_ci, float* slabs) {
#define LW_CASE(T)                                                                                                                            \
    case T:                                                                                                                                   \
        return YR_LAUNCH((lw_wgrad_partial_kernel<TA, T>), grid, dim3(256), 0, 0, s, ("lw_wgrad_partial_kernel<%d,%d>", TA, T), x, x_ld, dy, dy_ld, pixels, \
                         cin, cout, kp, chunk, per_co, per_ci, slabs);
    if constexpr (TA >= 3) {
        switch (tb) { LW_CASE(1) LW_CASE(2) LW_CASE(3) LW_CASE(4) }
    } else {
        switch (tb) { LW_CASE(3) LW_CASE(4) }
    }
#undef LW_CASE
    return YR_ERR_ARG;      // (not reached: tb is 1..4, and 3 or 4 where TA is 1 or 2 - a side above 256 has 6 to 8 tiles a block)
}

extern "C" int yr_linear_wide_wgrad(const float* x, int x_ld, const float* dy, int dy_ld, long long pixels, int cin, int cout, void* workspace,
                                    size_t workspace_bytes, float* dwt, void* stream) {
    YR_REQUIRE(x && dy && workspace && dwt, "linear_wide_wgrad: null pointer");
    YR_REQUIRE(lw_sizes_ok(pixels, cin, cout), "linear_wide_wgrad: pixels must be 1..2^40-1 and cin, cout 1..1024 (pixels %lld, cin %d, cout %d)", pixels, cin, cout);
    YR_REQUIRE(x_ld >= cin && dy_ld >= cout, "linear_wide_wgrad: x_ld %d < cin %d or dy_ld %d < cout %d", x_ld, cin, dy_ld, cout);
    YR_REQUIRE(tc_rows_fit(pixels, x_ld) && tc_rows_fit(pixels, dy_ld), "linear_wide_wgrad: byte offsets beyond 2^63");
    YR_REQUIRE(((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dwt) % 4 == 0, "linear_wide_wgrad: x, dy or dwt not 4-byte aligned");
    const int rc = tc_workspace_check("linear_wide_wgrad", workspace, workspace_bytes, yr_linear_wide_wgrad_workspace_bytes(pixels, cin, cout));
    if (rc != YR_OK) return rc;
    if (lw_narrow(cin, cout)) {      // (every refusal above is the narrow entry's too: it launches)
        yr_note_kernel("ht_wgrad_partial_kernel");
        return yr_linear_wgrad(x, x_ld, dy, dy_ld, pixels, cin, cout, workspace, workspace_bytes, dwt, stream);
    }
    const int kp = yr_round_up(cin, 4), chunk = lw_chunk(pixels, cin, cout);
    const int nchunks = (int)((pixels + chunk - 1) / chunk);
    int bo, po, bi, pi;
    lw_blocking(cout, LW_GW_TILES, &bo, &po);
    lw_blocking(cin, LW_GW_TILES, &bi, &pi);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(nchunks, bo, bi);
    float* slabs = (float*)workspace;
    const int tb = (pi + 1) / 2;
    int lrc = YR_OK;
    switch ((po + 1) / 2) {
        case 1: lrc = lw_wgrad_launch_ci<1>(tb, grid, s, x, x_ld, dy, dy_ld, pixels, cin, cout, kp, chunk, po, pi, slabs); break;
        case 2: lrc = lw_wgrad_launch_ci<2>(tb, grid, s, x, x_ld, dy, dy_ld, pixels, cin, cout, kp, chunk, po, pi, slabs); break;
        case 3: lrc = lw_wgrad_launch_ci<3>(tb, grid, s, x, x_ld, dy, dy_ld, pixels, cin, cout, kp, chunk, po, pi, slabs); break;
        default: lrc = lw_wgrad_launch_ci<4>(tb, grid, s, x, x_ld, dy, dy_ld, pixels, cin, cout, kp, chunk, po, pi, slabs); break;
    }
    if (lrc != YR_OK) return lrc;
    return yr_launch_slab_sum(slabs, nchunks, cout, kp, cin, dwt, s);
}
