// Pointwise (1x1) convolution on 16-bit activations and weights (bfloat16 / float16 storage, float32 accumulate):
// the reduced-precision form of pointwise.hip for BASELINE.json configs 3 and 5 ("bf16 pointwise on MFMA",
// "fp16 + fused RFCR upsample-concat-conv").  Same op, same fusions - UpSampling2D / MaxPooling2D / Concatenate /
// SE Multiply folded into the loads, BatchNorm scale/shift + activation + residual (+ 2x2 max) in the epilogue;
// reference code/yolo3/model.py:25-30,98-114,152-155,243-251,298-318, code/yolo3/efficientnet.py:485-496,517-533.
//
// GEMM view: D[cout][pixel] = sum_k Wt[cout][k] * X[pixel][k] on v_mfma_f32_16x16x32_bf16 / _f16:
//   A operand = weights  (lane l: cout row i = l&15, the 8 consecutive k of group g = l>>4: one 16-byte load)
//   B operand = pixels   (lane l: pixel j = l&15, the same 8 k)
//   D: lane holds pixel j = l&15, MFMA rows 4g..4g+3 (float32).
// The k space is the concatenation of the sources, each padded to a multiple of 8 channels (16 bytes), walked in
// chunks of 32.  Cout tiles come in PAIRS and the weight rows are assigned to MFMA rows so that row 4g+r of the pair's
// first tile is cout 8g+r and of its second tile cout 8g+4+r: lane group g then owns the 8 CONSECUTIVE couts
// 8g..8g+7 of a pixel - one 16-byte store of bf16/f16 (or two float4 stores for the float32 logit outputs).
// No LDS, no barriers (the direct form of pointwise.hip): every wave loads both operands straight into operand
// layout and keeps D chunks of loads in flight; the steady-state loop is branch-free so the waits are counted.
#include <stdlib.h>

#include "pwh_common.h"


// PT: 16-pixel tiles per wave, CP: 32-cout tile PAIRS per wave; 4 waves along the pixels: BM = 64*PT, BN = 32*CP.
template <class T, int PT, int CP, int D, int MODE>
__global__ __launch_bounds__(256) void pwh_kernel(PwArgs a) {
    constexpr int BM = 64 * PT, BN = 32 * CP, CT = 2 * CP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, li = lane & 15;
    const unsigned ntn = (a.N + BN - 1) / BN;
    const unsigned L = yr_xcd_swizzle(blockIdx.x, gridDim.x);
    const int m0 = (int)(L / ntn) * BM + wave * 16 * PT;
    const int n0 = (int)(L % ntn) * BN;
    const int kp = a.S.kp;
    const int kl = g * 8;  // this lane's k offset inside a 32-deep chunk

    PwhRow<MODE, T> row[PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) row[p].init(a, m0 + p * 16 + li);
    const T* brow[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        // MFMA row li of tile t <-> cout: see the header (lane group g ends up owning couts 8g..8g+7 of the pair)
        // (also in pwhp_kernel, pwhl_kernel, pwkh_kernel and mbh.hip: sharing it as a function changes the code of 44 kernels)
        const int n = n0 + (t >> 1) * 32 + 8 * (li >> 2) + 4 * (t & 1) + (li & 3);
        brow[t] = reinterpret_cast<const T*>(a.wt) + (size_t)(n < a.N ? n : 0) * kp;  // rows beyond N feed couts that are never stored
    }

    struct Frag {
        pwh_u4 x[PT], w[CT];
        float4 g0[MODE == 2 ? PT : 1], g1[MODE == 2 ? PT : 1];
        int cv[PT];
    };
    auto load = [&](auto pools_tag, int chunk, Frag& F) __attribute__((always_inline)) {
        constexpr bool POOLS = decltype(pools_tag)::value;
        const int kraw = chunk * 32 + kl;
#pragma unroll
        for (int p = 0; p < PT; ++p)
            row[p].template issue<POOLS>(a, kraw, kp, F.x[p], F.g0[MODE == 2 ? p : 0], F.g1[MODE == 2 ? p : 0], F.cv[p]);
        const int k = pw_kclamp<8>(kraw, kp);  // the k tail of the weights meets zeroed activations
#pragma unroll
        for (int t = 0; t < CT; ++t) F.w[t] = *reinterpret_cast<const pwh_u4*>(brow[t] + k);
    };

    f32x4 acc[CT][PT];
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int p = 0; p < PT; ++p) acc[t][p] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // uniform: most layers have whole octets and whole 32-deep chunks only, and then nothing needs masking
    const bool need_mask = MODE != 1 || (a.S.s[0].c & 7) != 0 || (kp & 31) != 0;

    auto use = [&](const Frag& F) __attribute__((always_inline)) {
        pwh_u4 xf[PT];
#pragma unroll
        for (int p = 0; p < PT; ++p)
            xf[p] = need_mask ? pwh_finish<MODE, T>(F.x[p], F.g0[MODE == 2 ? p : 0], F.g1[MODE == 2 ? p : 0], F.cv[p]) : F.x[p];
#pragma unroll
        for (int t = 0; t < CT; ++t)
#pragma unroll
            for (int p = 0; p < PT; ++p) acc[t][p] = pwh_mfma<T>(F.w[t], xf[p], acc[t][p]);
    };

    auto run = [&](auto pools_tag) __attribute__((always_inline)) {
        const int nch = (kp + 31) >> 5;  // chunk j lives in F[j % D]
        Frag F[D];
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (d < nch) load(pools_tag, d, F[d]);
        int j0 = 0;
        for (; j0 + 2 * D - 1 < nch; j0 += D) {  // steady state, branch-free: the whole next group exists
#pragma unroll
            for (int d = 0; d < D; ++d) {
                use(F[d]);
                load(pools_tag, j0 + D + d, F[d]);
            }
        }
#pragma unroll
        for (int t = 0; t < 2 * D - 1; ++t) {    // drain
            const int j = j0 + t;
            if (j < nch) {
                use(F[t % D]);
                if (j + D < nch) load(pools_tag, j + D, F[t % D]);
            }
        }
    };
    bool pooled = false;
    if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < YR_MAX_SRC; ++i)
            pooled |= a.S.s[i].xform == YR_X_MAXPOOL2 || a.S.s[i].xform == YR_X_MAXPOOL4;
    }
    if (pooled) run(std::true_type{});
    else run(std::false_type{});

    // ---- epilogue: lane group g owns couts 8g..8g+7 of every pair (tiles 2c and 2c+1) for its PT pixels
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        const int n = n0 + c * 32 + g * 8;
        float sc[8], sh[8];
        pwh_load_bn(a, n, sc, sh);
#pragma unroll
        for (int p = 0; p < PT; ++p) pwh_finish_oct<T>(a, acc[2 * c][p], acc[2 * c + 1][p], sc, sh, m0 + p * 16 + li, n, li);
    }
}

// Small-K form (k space of at most 32*NCH channels, one identity source, optional SE gate): the projections of the
// high-resolution blocks - [millions of pixels] x [32..128 channels] -> [16..48 couts].  In pwh_kernel a wave fetches its
// PT pixel tiles, multiplies and leaves: with a single 32-deep chunk there is nothing to pipeline INSIDE a tile set, so
// every workgroup's life is one exposed HBM round trip (EfficientNet-B0 stage 1 projection, 128 x 208 x 208 pixels:
// 0.29 ms at 1.85 TB/s).  Here a workgroup keeps the weight fragments of its cout tile in registers and WALKS a contiguous
// range of pixel tiles; the next tile's activations (and gate rows) are in flight while the current tile is multiplied
// and stored.  Same MFMA sequence per output as pwh_kernel: bit-identical results.
template <class T, int PT, int CP, int NCH, int MODE>
__global__ __launch_bounds__(256) void pwhp_kernel(PwArgs a, int tiles_per_wg) {
    static_assert(MODE == 1 || MODE == 2, "one identity source");
    constexpr int BM = 64 * PT, BN = 32 * CP, CT = 2 * CP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, li = lane & 15;
    const int n0 = (int)blockIdx.y * BN;
    const int kp = a.S.kp;
    const int kl = g * 8;
    const int ntm = (a.M + BM - 1) / BM;
    const int t_begin = (int)blockIdx.x * tiles_per_wg;
    const int t_end = t_begin + tiles_per_wg < ntm ? t_begin + tiles_per_wg : ntm;
    if (t_begin >= t_end) return;

    pwh_u4 wf[NCH][CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        const int n = n0 + (t >> 1) * 32 + 8 * (li >> 2) + 4 * (t & 1) + (li & 3);
        const T* brow = reinterpret_cast<const T*>(a.wt) + (size_t)(n < a.N ? n : 0) * kp;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const int kraw = ch * 32 + kl;
            wf[ch][t] = *reinterpret_cast<const pwh_u4*>(brow + pw_kclamp<8>(kraw, kp));
        }
    }
    float sc[CP][8], sh[CP][8];
#pragma unroll
    for (int c = 0; c < CP; ++c) pwh_load_bn(a, n0 + c * 32 + g * 8, sc[c], sh[c]);

    struct Tile {
        pwh_u4 x[NCH][PT];
        float4 g0[MODE == 2 ? NCH : 1][MODE == 2 ? PT : 1], g1[MODE == 2 ? NCH : 1][MODE == 2 ? PT : 1];
        int cv[NCH][PT];
    };
    auto fetch = [&](int mt, Tile& X) __attribute__((always_inline)) {
        const int m0 = mt * BM + wave * 16 * PT;
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            PwhRow<MODE, T> row;
            row.init(a, m0 + p * 16 + li);
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
                row.template issue<false>(a, ch * 32 + kl, kp, X.x[ch][p], X.g0[MODE == 2 ? ch : 0][MODE == 2 ? p : 0],
                                          X.g1[MODE == 2 ? ch : 0][MODE == 2 ? p : 0], X.cv[ch][p]);
        }
    };
    const bool need_mask = MODE != 1 || (a.S.s[0].c & 7) != 0 || (kp & 31) != 0 || kp < 32 * NCH;
    auto compute = [&](int mt, const Tile& X) __attribute__((always_inline)) {
        f32x4 acc[CT][PT];
#pragma unroll
        for (int t = 0; t < CT; ++t)
#pragma unroll
            for (int p = 0; p < PT; ++p) acc[t][p] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            pwh_u4 xf[PT];
#pragma unroll
            for (int p = 0; p < PT; ++p)
                xf[p] = need_mask ? pwh_finish<MODE, T>(X.x[ch][p], X.g0[MODE == 2 ? ch : 0][MODE == 2 ? p : 0],
                                                        X.g1[MODE == 2 ? ch : 0][MODE == 2 ? p : 0], X.cv[ch][p]) : X.x[ch][p];
#pragma unroll
            for (int t = 0; t < CT; ++t)
#pragma unroll
                for (int p = 0; p < PT; ++p) acc[t][p] = pwh_mfma<T>(wf[ch][t], xf[p], acc[t][p]);
        }
        const int m0 = mt * BM + wave * 16 * PT;
#pragma unroll
        for (int c = 0; c < CP; ++c)
#pragma unroll
            for (int p = 0; p < PT; ++p)
                pwh_finish_oct<T>(a, acc[2 * c][p], acc[2 * c + 1][p], sc[c], sh[c], m0 + p * 16 + li, n0 + c * 32 + g * 8, li);
    };
    Tile cur, nxt;
    fetch(t_begin, cur);
    for (int mt = t_begin; mt < t_end; ++mt) {
        if (mt + 1 < t_end) fetch(mt + 1, nxt);   // (uniform) the next tile's loads are in flight during this tile's MFMAs and stores
        compute(mt, cur);
        cur = nxt;                                // register moves: cheaper than a second copy of the multiply + epilogue code
    }
}

// LDS-tiled form: a workgroup computes up to 128 pixels x 128
// couts.  The direct kernel above re-fetches every operand fragment per wave - with PT = 4, CP = 1 six 1 KB loads per
// eight MFMAs - and the mid-size GEMMs of the unfused EfficientNet stages ([13k..51k pixels] x [136..1392] x [136..1392])
// ran at 1.0-1.7 TB/s whatever the tile shape (tools/pwh_probe.py): bound by the L1/L2 -> register path, not by HBM or
// the matrix pipe.  Here both operands of a 32-deep chunk are fetched once per workgroup (four 16-byte loads per thread),
// parked in LDS in FRAGMENT order - tile of 16 rows = 64 lanes x 16 bytes, lane (k group g, row i) at slot 16g + i, so
// the store of a wave's loads and every ds_read_b128 are linear, conflict-free - and each wave multiplies a 64 x 64
// sub-tile (4 + 4 fragment reads per 16 MFMAs).  Two LDS buffers, one barrier per chunk, the next chunk's global loads in
// flight during the MFMAs.  Same MFMA sequence and operand mapping per output as pwh_kernel: bit-identical results.
// PT x CT: 16 x 16 MFMA tiles per wave (pixels x couts); 2 x 2 waves: BM = 32 PT, BN = 32 CT.  MODE as in PwhRow: the
// pixel operand goes through the same row object as in pwh_kernel (gathers, pooled sources, SE gate and pad masking
// included) - only WHO fetches an octet differs: loader thread (row tid >> 2, k group tid & 3) instead of MFMA lane.
template <class T, int PT, int CT, int MODE, bool POOLS>
__global__ __launch_bounds__(256, 3) void pwhl_kernel(PwArgs a) {
    constexpr int BM = 32 * PT, BN = 32 * CT;
    constexpr int NWH = BN / 64, NXH = BM / 64;     // rows per loader thread
    __shared__ pwh_u4 frag[2][2 * CT + 2 * PT][64];   // [buffer][16-row tile: weights first, then pixels][fragment lane]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, li = lane & 15;
    const int wm = wave & 1, wn = wave >> 1;
    const unsigned ntn = (a.N + BN - 1) / BN;
    const unsigned L = yr_xcd_swizzle(blockIdx.x, gridDim.x);
    const int m0 = (int)(L / ntn) * BM, n0 = (int)(L % ntn) * BN;
    const int kp = a.S.kp, nch = (kp + 31) >> 5;

    // loader: thread (row r = tid >> 2, k group lg = tid & 3) fetches rows r, r + 64 .. of both operands
    const int lr = tid >> 2, lg = tid & 3;
    const T* wrow[NWH];
    PwhRow<MODE, T> xrow[NXH];
#pragma unroll
    for (int h = 0; h < NWH; ++h) {
        const int rho = lr + 64 * h, tile = rho >> 4, i = rho & 15;
        const int n = n0 + (tile >> 1) * 32 + 8 * (i >> 2) + 4 * (tile & 1) + (i & 3);   // MFMA row i of tile <-> cout: as in pwh_kernel
        wrow[h] = reinterpret_cast<const T*>(a.wt) + (size_t)(n < a.N ? n : 0) * kp;
    }
#pragma unroll
    for (int h = 0; h < NXH; ++h) xrow[h].init(a, m0 + lr + 64 * h);
    const int slot = (lr >> 4) * 64 + lg * 16 + (lr & 15);   // + 256 per further 64 rows
    // uniform: most layers have whole octets and whole 32-deep chunks only, and then nothing needs masking
    const bool need_mask = MODE != 1 || (a.S.s[0].c & 7) != 0 || (kp & 31) != 0;
    struct Stage {
        pwh_u4 w[NWH], x[NXH];
        float4 g0[MODE == 2 ? NXH : 1], g1[MODE == 2 ? NXH : 1];
        int cv[NXH];
    };
    auto fetch = [&](int chunk, Stage& R) __attribute__((always_inline)) {
        const int kraw = chunk * 32 + lg * 8;
        const int k = pw_kclamp<8>(kraw, kp);   // the k tail of the weights meets zeroed activations
#pragma unroll
        for (int h = 0; h < NWH; ++h) R.w[h] = *reinterpret_cast<const pwh_u4*>(wrow[h] + k);
#pragma unroll
        for (int h = 0; h < NXH; ++h)
            xrow[h].template issue<POOLS>(a, kraw, kp, R.x[h], R.g0[MODE == 2 ? h : 0], R.g1[MODE == 2 ? h : 0], R.cv[h]);
    };
    auto park = [&](int buf, const Stage& R) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < NWH; ++h) (&frag[buf][0][0])[slot + 256 * h] = R.w[h];
#pragma unroll
        for (int h = 0; h < NXH; ++h)
            (&frag[buf][2 * CT][0])[slot + 256 * h] =
                need_mask ? pwh_finish<MODE, T>(R.x[h], R.g0[MODE == 2 ? h : 0], R.g1[MODE == 2 ? h : 0], R.cv[h]) : R.x[h];
    };

    f32x4 acc[CT][PT];
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int p = 0; p < PT; ++p) acc[t][p] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto multiply = [&](int buf) __attribute__((always_inline)) {
        pwh_u4 w[CT], x[PT];
#pragma unroll
        for (int t = 0; t < CT; ++t) w[t] = frag[buf][wn * CT + t][lane];
#pragma unroll
        for (int p = 0; p < PT; ++p) x[p] = frag[buf][2 * CT + wm * PT + p][lane];
#pragma unroll
        for (int t = 0; t < CT; ++t)
#pragma unroll
            for (int p = 0; p < PT; ++p) acc[t][p] = pwh_mfma<T>(w[t], x[p], acc[t][p]);
    };

    // chunk c is multiplied out of LDS buffer c & 1 while chunk c + 1 is in flight into registers.  One barrier per chunk:
    // the buffer parked into during chunk c is the one chunk c - 1 was read from, and everyone has passed the barrier
    // since.  (A second register stage - chunk c + 2 in flight as well - costs 10 VGPRs = one wave per SIMD on the 128 x 64
    // tile and measured 10-20 % SLOWER: waves in flight hide more latency than loads in flight per wave; three or four
    // stages did not win on the long-k projections of the 20 x 20 maps either - tools/pwh_probe.py.)
    Stage R;
    fetch(0, R);
    park(0, R);
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        if (c + 1 < nch) fetch(c + 1, R);   // (uniform)
        multiply(c & 1);
        if (c + 1 < nch) park((c & 1) ^ 1, R);
        __syncthreads();
    }

#pragma unroll
    for (int c = 0; c < CT / 2; ++c) {
        const int n = n0 + wn * 16 * CT + c * 32 + g * 8;
        float sc[8], sh[8];
        pwh_load_bn(a, n, sc, sh);
#pragma unroll
        for (int p = 0; p < PT; ++p) pwh_finish_oct<T>(a, acc[2 * c][p], acc[2 * c + 1][p], sc, sh, m0 + wm * 16 * PT + p * 16 + li, n, li);
    }
}

template <class T, int PT, int CT>
static int launch_lds(const PwArgs& a, hipStream_t s) {
    if (a.dw_w) { yr_set_error("pointwise: the depthwise-folded source is a float32 feature"); return YR_ERR_ARG; }
    int mode;
    if (int rc = pw_mode(a, &mode)) return rc;
    // (names spelled like the symbols: element type, PT, CT, MODE, POOLS)
#define PWHL_GO(MODE, POOLS) YR_LAUNCH((pwhl_kernel<T, PT, CT, MODE, POOLS>), pw_grid(a, 32 * PT, 32 * CT), dim3(256), 0, 0, s, ("pwhl_kernel<%s,%d,%d,%d,%d>", yr_dtype_name(yr_elem<T>::dtype), PT, CT, MODE, POOLS), a)
    return mode == 1 ? PWHL_GO(1, 0) : mode == 2 ? PWHL_GO(2, 0) : pw_any_pooled(a.S) ? PWHL_GO(0, 1) : PWHL_GO(0, 0);
#undef PWHL_GO
}

template <class T, int PT, int CP, int NCH>
static int launch_hp(const PwArgs& a, int mode, hipStream_t s) {
    constexpr int BM = 64 * PT, BN = 32 * CP;
    const int ntm = (a.M + BM - 1) / BM, ntn = (a.N + BN - 1) / BN;
    // about 8 workgroups per CU in flight and at least 4 tiles per workgroup (the first tile's fetch is exposed)
    int per = (ntm + 2047) / 2048;
    if (per < 4) per = 4;
    const int wgs = (ntm + per - 1) / per;
    const dim3 grid((unsigned)wgs, (unsigned)ntn);
#define PWHP_GO(MODE) YR_LAUNCH((pwhp_kernel<T, PT, CP, NCH, MODE>), grid, dim3(256), 0, 0, s, ("pwhp_kernel<%s,%d,%d,%d,%d>", yr_dtype_name(yr_elem<T>::dtype), PT, CP, NCH, MODE), a, per)
    return mode == 1 ? PWHP_GO(1) : PWHP_GO(2);
#undef PWHP_GO
}

template <class T, int PT, int CP>
static int launch_h(const PwArgs& a, hipStream_t s) {
    // chunks of loads in flight; four pixel tiles per wave keep two (three spilled 464-544 bytes per lane in the f16 gather form)
    constexpr int D = PT >= 4 ? 2 : (PT + 2 * CP <= 4 ? 4 : (PT + 2 * CP <= 8 ? 3 : 2));
    int mode;
    if (int rc = pw_mode(a, &mode)) return rc;
#define PWH_GO(MODE) YR_LAUNCH((pwh_kernel<T, PT, CP, D, MODE>), pw_grid(a, 64 * PT, 32 * CP), dim3(256), 0, 0, s, ("pwh_kernel<%s,%d,%d,%d,%d>", yr_dtype_name(yr_elem<T>::dtype), PT, CP, D, MODE), a)
    return PW_BY_MODE(mode, PWH_GO);
#undef PWH_GO
}

// the small-K walking form (pwhp_kernel); where it does not apply (more than 128 k, gathered sources) the plain kernel of the same
// tile shape runs, so every index is valid for every op
template <class T, int PT, int CP>
static int launch_walk(const PwArgs& a, hipStream_t s) {
    const int mode = pw_mode_of(a);
    const int nch = (a.S.kp + 31) >> 5;
    if (mode == 0 || nch > 4 || a.dw_w != nullptr) return launch_h<T, PT, CP>(a, s);
    if (nch <= 1) return launch_hp<T, PT, CP, 1>(a, mode, s);
    if (nch <= 2) return launch_hp<T, PT, CP, 2>(a, mode, s);
    return launch_hp<T, PT, CP, 4>(a, mode, s);
}

// ---- THE TILE SHAPES of the 16-bit kernels, index = position in the lists taken one after the other (the tuner's op.k - 1):
// the direct kernel, X(PT, CP, launcher): BM = 64 PT, BN = 32 CP - the shapes the heuristic ranks (the direct kernel of the
// 128 x 128 shape spilled 272 bytes per lane: that index runs its LDS-tiled twin, launch_lds<T, 2, 4>);
#define PWH_DIRECT_SHAPES(X)                                                                                              \
    X(1, 1, launch_h) X(1, 2, launch_h) X(1, 3, launch_h) X(1, 4, launch_h) X(2, 1, launch_h) X(2, 2, launch_h) X(2, 3, launch_h) \
    X(2, 4, launch_lds) X(4, 1, launch_h) X(4, 2, launch_h)
// the small-K walking form in four of those shapes, and the LDS-tiled form (pwhl_kernel), X(PT, CT): BM = 32 PT, BN = 32 CT;
#define PWH_WALK_SHAPES(X) X(1, 1) X(2, 1) X(1, 2) X(2, 2)
#define PWH_LDS_SHAPES(X) X(4, 4) X(2, 4) X(4, 2) X(2, 2)
// then the activation-stationary form (pointwise_hs.hip, k <= 256) and the all-couts k-streaming form (pointwise_hq.hip) in
// PWH_NVARIANT variants each; ops they do not take run the 128 x 64 LDS-tiled shape
constexpr int PWH_NVARIANT = 4;
struct PwhCfg { int bm, bn; };
#define PWH_CFG(PT, CP, FN) {64 * PT, 32 * CP},
static const PwhCfg pwh_cfgs[] = {PWH_DIRECT_SHAPES(PWH_CFG)};
constexpr int PWH_NCFG = sizeof(pwh_cfgs) / sizeof(pwh_cfgs[0]);
constexpr int PWH_NWALK = 0 PWH_WALK_SHAPES(PW_COUNT) PWH_LDS_SHAPES(PW_COUNT);
constexpr int PWH_NSQ = 2 * PWH_NVARIANT;
int yr_pwh_num_cfgs() { return PWH_NCFG + PWH_NWALK + PWH_NSQ; }

template <class T>
static int launch_h_cfg(int cfg, const PwArgs& a, hipStream_t s) {
    typedef int (*Fn)(const PwArgs&, hipStream_t);
#define PWH_FN_H(PT, CP, FN) FN<T, PT, CP>,
#define PWH_FN_W(PT, CP) launch_walk<T, PT, CP>,
#define PWH_FN_L(PT, CT) launch_lds<T, PT, CT>,
    static const Fn fns[] = {PWH_DIRECT_SHAPES(PWH_FN_H) PWH_WALK_SHAPES(PWH_FN_W) PWH_LDS_SHAPES(PWH_FN_L)};
    if (cfg >= 0 && cfg < PWH_NCFG + PWH_NWALK) return fns[cfg](a, s);
    YR_REQUIRE(cfg >= 0 && cfg < PWH_NCFG + PWH_NWALK + PWH_NSQ, "pointwise: 16-bit tile shape %d out of range", cfg);
    const int v = cfg - (PWH_NCFG + PWH_NWALK);
    const int rc = v < PWH_NVARIANT ? yr_pwhs_launch(yr_elem<T>::dtype, v, a, s) : yr_pwhq_launch(yr_elem<T>::dtype, v - PWH_NVARIANT, a, s);
    return rc == YR_NOT_TAKEN ? launch_lds<T, 4, 2>(a, s) : rc;
}

// The K-SPLIT form for the passes of one or two images (YR_PWF_KSPLIT on a POINTWISE op, set by the compiler's 'latency' variant of
// a 16-bit plan for its small maps; the float32 twin is pointwise_split.hip's pwk_kernel).  pwh_kernel gives a wave 16 pixels x 32
// couts and the whole k range: at 169 .. 1024 pixels a gated projection of 1152 channels is 36 chunks behind each other (9.8 us at
// one image).  Here a workgroup is ONE such tile and its four waves take the chunks w, w + 4, ... (PWKH_G of them in flight per wave);
// the four accumulator pairs meet in LDS in wave order and wave 0 runs pwh_kernel's epilogue.
#define PWKH_G 3
template <class T, int MODE>
__global__ __launch_bounds__(256) void pwkh_kernel(PwArgs a) {
    __shared__ f32x4 red[3][2][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, li = lane & 15;
    const unsigned ntn = (a.N + 31) / 32;
    const unsigned L = yr_xcd_swizzle(blockIdx.x, gridDim.x);
    const int m0 = (int)(L / ntn) * 16, n0 = (int)(L % ntn) * 32;
    const int kp = a.S.kp, nch = (kp + 31) >> 5;
    PwhRow<MODE, T> row;
    row.init(a, m0 + li);
    const T* brow[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n = n0 + 8 * (li >> 2) + 4 * t + (li & 3);   // (pwh_kernel's row assignment: lane group g ends up owning couts 8 g .. 8 g + 7)
        brow[t] = reinterpret_cast<const T*>(a.wt) + (size_t)(n < a.N ? n : 0) * kp;
    }
    f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
    auto run = [&](auto pools_tag) __attribute__((always_inline)) {
        constexpr bool POOLS = decltype(pools_tag)::value;
        for (int c0 = wave; c0 < nch; c0 += 4 * PWKH_G) {
            pwh_u4 x[PWKH_G], w[PWKH_G][2];
            float4 g0[PWKH_G], g1[PWKH_G];
            int cv[PWKH_G];
            pw_unroll<PWKH_G>([&](auto J) __attribute__((always_inline)) {
                constexpr int j = decltype(J)::value;
                const int kraw = (c0 + 4 * j) * 32 + g * 8;       // (beyond kp for a dead chunk: clamped addresses, cv = 0)
                row.template issue<POOLS>(a, kraw, kp, x[j], g0[j], g1[j], cv[j]);
                const int k = pw_kclamp<8>(kraw, kp);
                w[j][0] = *reinterpret_cast<const pwh_u4*>(brow[0] + k);
                w[j][1] = *reinterpret_cast<const pwh_u4*>(brow[1] + k);
            });
            pw_unroll<PWKH_G>([&](auto J) __attribute__((always_inline)) {
                constexpr int j = decltype(J)::value;
                if (c0 + 4 * j < nch) {      // (wave-uniform)
                    const pwh_u4 xf = pwh_finish<MODE, T>(x[j], g0[j], g1[j], cv[j]);
                    acc[0] = pwh_mfma<T>(w[j][0], xf, acc[0]);
                    acc[1] = pwh_mfma<T>(w[j][1], xf, acc[1]);
                }
            });
        }
    };
    bool pooled = false;
    if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < YR_MAX_SRC; ++i)
            pooled |= a.S.s[i].xform == YR_X_MAXPOOL2 || a.S.s[i].xform == YR_X_MAXPOOL4;
    }
    if (pooled) run(std::true_type{});
    else run(std::false_type{});
    if (wave > 0) { red[wave - 1][0][lane] = acc[0]; red[wave - 1][1][lane] = acc[1]; }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < 3; ++w) { acc[0] += red[w][0][lane]; acc[1] += red[w][1][lane]; }   // (in wave order)
    const int n = n0 + g * 8;
    float sc[8], sh[8];
    pwh_load_bn(a, n, sc, sh);
    pwh_finish_oct<T>(a, acc[0], acc[1], sc, sh, m0 + li, n, li);
}

template <class T>
static int launch_ksplit_t(const PwArgs& a, hipStream_t s) {
    int mode;
    if (int rc = pw_mode(a, &mode)) return rc;
#define PWKH_GO(MODE) YR_LAUNCH((pwkh_kernel<T, MODE>), pw_grid(a, 16, 32), dim3(256), 0, 0, s, ("pwkh_kernel<%s,%d>", yr_dtype_name(yr_elem<T>::dtype), MODE), a)
    return PW_BY_MODE(mode, PWKH_GO);
#undef PWKH_GO
}
int yr_pwh_launch_ksplit(int dtype, const PwArgs& a, hipStream_t s) { return PWH_BY_DTYPE(dtype, pwh_bad_dtype(dtype), launch_ksplit_t, a, s); }

// 16-bit ops: a filled PwArgs (yr_launch_pointwise did the argument checks that do not depend on the element type);
// cfg = op.k - 1 (autotuned tile shape) or -1: heuristic.
// the heuristic's pick among the direct shapes, a pure function of the GEMM's extents: the widest cout tile that still yields ~2
// workgroups per CU, 128-row tiles when pixels abound
static int pwh_pick_cfg(int M, int N, int kp) {
    const double Md = (double)M;
    double best = 1e30;
    int cfg = -1;
    for (int i = 0; i < PWH_NCFG; ++i) {
        const PwhCfg& c = pwh_cfgs[i];
        const double ntn = (double)((N + c.bn - 1) / c.bn), nblk = (double)((M + c.bm - 1) / c.bm) * ntn;
        const double t_mem = Md * kp * 2.0 * (1.0 + 0.25 * (ntn - 1.0)) + Md * N * 2.0 + nblk * c.bn * kp * 2.0 * 0.25;
        const double fill = nblk < 512.0 ? 512.0 / nblk : 1.0;
        const double regs = (c.bm / 64) * (c.bn / 16) > 16 ? 1.3 : 1.0;
        const double cost = t_mem * fill * regs;
        if (cost < best) { best = cost; cfg = i; }
    }
    return cfg;
}

int yr_pw_launch_h(int dtype, int cfg, const PwArgs& a, hipStream_t s) {
    if (cfg < 0 || cfg >= PWH_NCFG + PWH_NWALK + PWH_NSQ) cfg = pwh_pick_cfg(a.M, a.N, a.S.kp);
    return PWH_BY_DTYPE(dtype, pwh_bad_dtype(dtype), launch_h_cfg, cfg, a, s);
}
