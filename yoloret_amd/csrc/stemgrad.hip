// The network entry as a training operator: a dense 3 x 3 convolution, 1..4 -> 1..64 channels, stride 1 or 2, with its two gradients.
// It is MobileNetV2's Conv1 (reference code/yolo3/model.py:180,193: tf.keras.applications.MobileNetV2, Conv2D(first, 3, strides 2,
// 'same', no bias) on the image) and EfficientNet's stem_conv (reference code/yolo3/efficientnet.py: Conv2D(round_filters(32), 3,
// strides 2, 'same', no bias)): the one layer of the backbones that is neither a 1x1 nor a depthwise convolution.  The reference
// trains it with every other layer (code/train.py:150-216); its backward is TensorFlow's tape.  yoloret_amd/autograd.py wires the
// entries into torch.autograd (conv3x3); tests/stemgrad_ref.py is the definition.
//
// The conventions are those of train_common.h and of the depthwise entries of convgrad.hip: maps [B][H][W][ld], explicit pad_top,
// pad_left in 0..2 and the output size (OH, OW), which must be floor((H + pad_top + pad_bottom - 3) / stride) + 1 for some pad_bottom
// in 0..2 (columns alike).  The weight is the Keras kernel [3, 3, cin, cout] as it lies in memory: w[(ky * 3 + kx) * cin + ci][cout],
// dense rows of cout floats.  At the workload (64 x 416 x 416 x 3 -> 208 x 208 x 24) an entry moves 400 MB for 648 FMAs per output
// pixel, 1.8 G in all - far below the VALU's rate -, so these are plain VALU kernels whose weights never pass through VGPR loads:
// every weight index is the same in all lanes and is read through the constant address space (s_load: an SGPR operand of the fmaf),
// as the inference entry kernels (stemblock.hip) do.  Measured: the forward and the input gradient run at about
// 2 x a copy of their bytes, the weight gradient at 6 x - its register tile is too small for its operand traffic; a tile staged
// through LDS is the known next step.
//
// THE ORDER.  One IEEE float32 fmaf per (tap, channel) term and nothing else, every chain from +0:
//   forward  y[b][oy][ox][co]: for ky in 0..2, for kx in 0..2, for ci in 0..cin-1:
//                acc = fmaf(x[b][oy s - pt + ky][ox s - pl + kx][ci], w[(ky * 3 + kx) * cin + ci][co], acc)
//   dgrad    dx[b][iy][ix][ci]: for ky in 0..2, for kx in 0..2 with iy + pt - ky = oy s and ix + pl - kx = ox s, for co in 0..cout-1:
//                acc = fmaf(dy[b][oy][ox][co], w[(ky * 3 + kx) * cin + ci][co], acc)
//   THE PAD RULE: a tap that falls outside the map (forward, wgrad) or whose output pixel does not exist (dgrad) is SKIPPED - no
//   operation at all, not an fmaf with a zero: a chain that has underflowed to -0 keeps its -0, and an input pixel no window touches
//   gets the untouched +0.  Every dx[..][0..cin) is written.
//   wgrad    dw[r][co], r = (ky * 3 + kx) * cin + ci.  The B * OH output rows are cut into chunks of yr_conv3x3_wgrad_chunk(B, OH, OW,
//            cin, cout) rows; a chunk's pixels are numbered i = 0, 1, .. in (row, column) order.  With Q = ceil(cout / 4) channel
//            quads, a workgroup of 256 lanes holds NS = 256 / round_up(9 Q, 64) sets (4 up to cout 28, 2 up to 56, else 1); set s
//            adds the pixels i = s, s + NS, s + 2 NS, .. in that order: acc = fmaf(dy[..][co], x[..][ci], acc), padded taps
//            skipped.  The sets' sums are then added in set order, ((s0 + s1) + s2) + s3, which is the chunk's slab; stage 2
//            (yr_launch_slab_sum) adds the slabs in index order and writes every dw element.
//
// Forms.  forward: a lane owns one output pixel and all its cout accumulators (CT = cout rounded up to 8, 64 for a cout that is no
//   multiple of 8: the guarded form); its up to 36 inputs are loaded first, then 9 cin rows of weights stream through SGPRs.  The
//   lane stores its row as 16-byte pieces.
// dgrad: a lane owns the s x s input pixels of one cell of the PADDED input grid, (s qy + a - pt, s qx + b - pl), whose taps are
//   the same in every lane: ky = a + s my meets output row qy - my.  It walks the ceil(3 / s)^2 output pixels (my, mx) ascending -
//   which is (ky, kx) ascending for each of its pixels -, loads that pixel's cout gradients once and feeds all its pixels' chains:
//   at stride 2 four loads of a dy row for four input pixels and no idle tap.
// wgrad: lane = (tap, channel quad) with cin x 4 accumulators in registers over the whole chunk: per pixel one 16-byte load of dy
//   and cin dwords of x for 4 cin FMAs.
#include "train_common.h"

#define SG_MIN_PIXELS 256     // output pixels per workgroup of the weight gradient, at least
#define SG_MAX_CHUNKS 2048
#define SG_MAX_CIN 4
#define SG_MAX_COUT 64

typedef const float __attribute__((address_space(4))) * sg_kptr;      // uniform reads of this become s_load
typedef float sg_f4u __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes at a dword-aligned address

struct sg_geo {
    int B, H, W, cin, cout, OH, OW, pt, pl, stride;
    long long x_ld, y_ld;      // leading dimensions of the input-side map (x / dx) and of the output-side map (y / dy)
};

// on = floor((n + pad + far - 3) / stride) + 1 for some far pad in 0..2 (the smallest that gives on outputs)
static inline bool sg_out_ok(int n, int on, int stride, int pad) {
    long long far = (long long)(on - 1) * stride + 3 - pad - n;
    if (far < 0) far = 0;
    return far <= 2 && n + pad + far - 3 < (long long)on * stride;
}

static int sg_check(const char* who, int B, int H, int W, int cin, int cout, int stride, int pt, int pl, int OH, int OW, int x_ld, int y_ld) {
    YR_REQUIRE(cin >= 1 && cin <= SG_MAX_CIN && cout >= 1 && cout <= SG_MAX_COUT, "%s: cin must be 1..4 and cout 1..64 (cin %d, cout %d)", who, cin, cout);
    YR_REQUIRE(stride == 1 || stride == 2, "%s: stride must be 1 or 2 (%d)", who, stride);
    YR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1, "%s: B, H, W, OH, OW must be positive", who);
    YR_REQUIRE(B <= 65535 && H <= 65535 && W <= 65535 && OH <= 65535 && OW <= 65535, "%s: B, H, W, OH or OW above 65535", who);
    YR_REQUIRE(pt >= 0 && pt < 3 && pl >= 0 && pl < 3, "%s: pad_top %d / pad_left %d outside 0..2", who, pt, pl);
    YR_REQUIRE(x_ld >= cin && y_ld >= cout, "%s: a leading dimension below the channels (x_ld %d, cin %d, y_ld %d, cout %d)", who, x_ld, cin, y_ld, cout);
    YR_REQUIRE(sg_out_ok(H, OH, stride, pt) && sg_out_ok(W, OW, stride, pl),
               "%s: output %d x %d is not what input %d x %d, stride %d, pads (%d, %d) and a bottom / right pad in 0..2 give", who, OH, OW, H, W, stride, pt, pl);
    const long long in = (long long)B * H * W, out = (long long)B * OH * OW;
    YR_REQUIRE(in * x_ld < (1ll << 40) && out * y_ld < (1ll << 40) && in <= (long long)INT_MAX * 64 && out <= (long long)INT_MAX * 64, "%s: map too large", who);
    return YR_OK;
}

// ---------------------------------------------------------------- forward
// EXACT: cout == CT (a multiple of 8): no channel guard.  Otherwise CT = 64, the weight index is clamped and every store asks co < cout.
template <int CT, bool EXACT>
__global__ __launch_bounds__(256) void sg_forward_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, sg_geo d) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;      // output pixel (b, oy, ox)
    const long long total = (long long)d.B * d.OH * d.OW;
    if (p >= total) return;
    const int ox = (int)(p % d.OW);
    const long long row = p / d.OW;
    const int oy = (int)(row % d.OH), b = (int)(row / d.OH);
    const int iy0 = oy * d.stride - d.pt, ix0 = ox * d.stride - d.pl;
    const int cin = d.cin, cout = d.cout;
    const sg_kptr wk = (sg_kptr)w;
    float xs[9][SG_MAX_CIN];
    bool ok[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int iy = iy0 + ky, ix = ix0 + kx;
            const bool in = iy >= 0 && iy < d.H && ix >= 0 && ix < d.W;
            ok[ky * 3 + kx] = in;
            const float* px = x + (((long long)b * d.H + (in ? iy : 0)) * d.W + (in ? ix : 0)) * d.x_ld;      // (a valid address either way)
#pragma unroll
            for (int ci = 0; ci < SG_MAX_CIN; ++ci) xs[ky * 3 + kx][ci] = ci < cin ? px[ci] : 0.f;
        }
    }
    float acc[CT];
#pragma unroll
    for (int co = 0; co < CT; ++co) acc[co] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        if (!ok[t]) continue;      // THE PAD RULE: skipped
#pragma unroll
        for (int ci = 0; ci < SG_MAX_CIN; ++ci) {
            if (ci >= cin) break;      // (the same in every lane)
            const sg_kptr wr = wk + (t * cin + ci) * cout;
            const float xv = xs[t][ci];
#pragma unroll
            for (int co = 0; co < CT; ++co) {
                const float wv = wr[EXACT || co < cout ? co : cout - 1];      // (guarded form: a valid address; channels past cout are not stored)
                acc[co] = __builtin_fmaf(xv, wv, acc[co]);
            }
        }
    }
    float* py = y + p * d.y_ld;
    if (EXACT) {
#pragma unroll
        for (int co = 0; co < CT; co += 4) *(sg_f4u*)(py + co) = (sg_f4u){acc[co], acc[co + 1], acc[co + 2], acc[co + 3]};
    } else {
#pragma unroll
        for (int co = 0; co < CT; ++co)
            if (co < cout) py[co] = acc[co];
    }
}

// ---------------------------------------------------------------- the input gradient
template <int S, int CT, bool EXACT>
__global__ __launch_bounds__(256) void sg_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx, sg_geo d, int QH, int QW) {
    constexpr int M = (3 + S - 1) / S;      // output pixels a cell's taps reach, per axis
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;      // cell (b, qy, qx) of the padded input grid
    if (q >= (long long)d.B * QH * QW) return;
    const int qx = (int)(q % QW);
    const long long qrow = q / QW;
    const int qy = (int)(qrow % QH), b = (int)(qrow / QH);
    const int cin = d.cin, cout = d.cout;
    const sg_kptr wk = (sg_kptr)w;
    float acc[S][S][SG_MAX_CIN];
#pragma unroll
    for (int a = 0; a < S; ++a)
#pragma unroll
        for (int c = 0; c < S; ++c)
#pragma unroll
            for (int ci = 0; ci < SG_MAX_CIN; ++ci) acc[a][c][ci] = 0.f;
#pragma unroll
    for (int my = 0; my < M; ++my) {
#pragma unroll
        for (int mx = 0; mx < M; ++mx) {
            const int oy = qy - my, ox = qx - mx;
            const bool in = oy >= 0 && oy < d.OH && ox >= 0 && ox < d.OW;
            const float* pd = dy + (((long long)b * d.OH + (in ? oy : 0)) * d.OW + (in ? ox : 0)) * d.y_ld;      // (a valid address either way)
            float g[EXACT ? CT : 1];      // (the guarded form reads dy inside its rolled chains)
            if (EXACT) {
#pragma unroll
                for (int co = 0; co < CT; co += 4) {
                    const sg_f4u v = *(const sg_f4u*)(pd + co);
                    g[co] = v.x; g[co + 1] = v.y; g[co + 2] = v.z; g[co + 3] = v.w;
                }
            }
            if (!in) continue;      // THE PAD RULE: skipped
#pragma unroll
            for (int a = 0; a < S; ++a) {
                const int ky = a + S * my;
                if (ky >= 3) continue;
#pragma unroll
                for (int c = 0; c < S; ++c) {
                    const int kx = c + S * mx;
                    if (kx >= 3) continue;
#pragma unroll
                    for (int ci = 0; ci < SG_MAX_CIN; ++ci) {
                        if (ci >= cin) break;      // (the same in every lane)
                        const sg_kptr wr = wk + ((ky * 3 + kx) * cin + ci) * cout;
                        float r = acc[a][c][ci];
                        if (EXACT) {
#pragma unroll
                            for (int co = 0; co < CT; ++co) r = __builtin_fmaf(g[co], wr[co], r);
                        } else {
                            for (int co = 0; co < cout; ++co) r = __builtin_fmaf(pd[co], wr[co], r);
                        }
                        acc[a][c][ci] = r;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < S; ++a) {
        const int iy = qy * S + a - d.pt;
        if (iy < 0 || iy >= d.H) continue;
#pragma unroll
        for (int c = 0; c < S; ++c) {
            const int ix = qx * S + c - d.pl;
            if (ix < 0 || ix >= d.W) continue;
            float* px = dx + (((long long)b * d.H + iy) * d.W + ix) * d.x_ld;
#pragma unroll
            for (int ci = 0; ci < SG_MAX_CIN; ++ci)
                if (ci < cin) px[ci] = acc[a][c][ci];
        }
    }
}

// ---------------------------------------------------------------- the weight gradient
static inline int sg_quads(int cout) { return (cout + 3) / 4; }
static inline int sg_set_lanes(int cout) { return yr_round_up(9 * sg_quads(cout), 64); }

static inline bool sg_sizes_ok(int B, int OH, int OW, int cin, int cout) {
    return B >= 1 && B <= 65535 && OH >= 1 && OH <= 65535 && OW >= 1 && OW <= 65535 && cin >= 1 && cin <= SG_MAX_CIN && cout >= 1 && cout <= SG_MAX_COUT &&
           (long long)B * OH * OW <= (long long)INT_MAX * 64;
}

// output rows (of the B * OH) per workgroup of stage 1
static inline int sg_chunk(int B, int OH, int OW) { return (int)tc_chunk((long long)B * OH, (SG_MIN_PIXELS + OW - 1) / OW, SG_MAX_CHUNKS); }

extern "C" int yr_conv3x3_wgrad_chunk(int B, int OH, int OW, int cin, int cout) { return sg_sizes_ok(B, OH, OW, cin, cout) ? sg_chunk(B, OH, OW) : 0; }

extern "C" size_t yr_conv3x3_wgrad_workspace_bytes(int B, int OH, int OW, int cin, int cout) {
    if (!sg_sizes_ok(B, OH, OW, cin, cout)) return 0;
    const long long chunk = sg_chunk(B, OH, OW), rows = (long long)B * OH;
    return (size_t)((rows + chunk - 1) / chunk) * (size_t)(9 * cin) * (size_t)cout * sizeof(float);
}

__global__ __launch_bounds__(256) void sg_wgrad_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ slabs, sg_geo d,
                                                               int chunk, int set_lanes) {
    __shared__ float red[192 * SG_MAX_CIN * 4];      // one set's accumulators: at most 144 items x 16
    const int cin = d.cin, cout = d.cout;
    const int quads = (cout + 3) / 4, items = 9 * quads, nsets = 256 / set_lanes;
    const int set = threadIdx.x / set_lanes, item = threadIdx.x - set * set_lanes;
    const bool live = set < nsets && item < items;
    const int t = live ? item / quads : 0, co0 = live ? (item - t * quads) * 4 : 0;
    const int ky = t / 3, kx = t - ky * 3;
    const bool whole = co0 + 4 <= cout;
    const long long rows = (long long)d.B * d.OH;
    const long long r0 = (long long)blockIdx.x * chunk;
    const long long r1 = r0 + chunk < rows ? r0 + chunk : rows;
    const long long n = (r1 - r0) * d.OW;      // output pixels of this chunk
    float acc[SG_MAX_CIN][4];
#pragma unroll
    for (int ci = 0; ci < SG_MAX_CIN; ++ci)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[ci][j] = 0.f;
    if (live) {
        // this set's pixels set, set + nsets, .. of the chunk, walked as (image, row, column): no division in the loop
        int ox = set % d.OW;
        long long row = r0 + set / d.OW;
        int b = (int)(row / d.OH), oy = (int)(row % d.OH);
        for (long long i = set; i < n; i += nsets, ox += nsets) {
            while (ox >= d.OW) {
                ox -= d.OW;
                ++row;
                if (++oy == d.OH) { oy = 0; ++b; }
            }
            const int iy = oy * d.stride - d.pt + ky, ix = ox * d.stride - d.pl + kx;
            const bool in = iy >= 0 && iy < d.H && ix >= 0 && ix < d.W;
            const float* px = x + (((long long)b * d.H + (in ? iy : 0)) * d.W + (in ? ix : 0)) * d.x_ld;      // (a valid address either way)
            const float* pd = dy + (row * d.OW + ox) * d.y_ld + co0;
            float g[4], xv[SG_MAX_CIN];
            if (whole) {
                const sg_f4u v = *(const sg_f4u*)pd;
                g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] = co0 + j < cout ? pd[j] : 0.f;
            }
#pragma unroll
            for (int ci = 0; ci < SG_MAX_CIN; ++ci) xv[ci] = ci < cin ? px[ci] : 0.f;
#pragma unroll
            for (int ci = 0; ci < SG_MAX_CIN; ++ci)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[ci][j] = in ? __builtin_fmaf(g[j], xv[ci], acc[ci][j]) : acc[ci][j];      // THE PAD RULE: skipped
        }
    }
    for (int s = 0; s < nsets; ++s) {      // the sets' sums, added in set order
        if (live && set == s) {
#pragma unroll
            for (int ci = 0; ci < SG_MAX_CIN; ++ci)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float* slot = red + (ci * 4 + j) * 192 + item;
                    *slot = s == 0 ? acc[ci][j] : *slot + acc[ci][j];
                }
        }
        __syncthreads();
    }
    if (live && set == 0) {
        float* slab = slabs + (size_t)blockIdx.x * (size_t)(9 * cin) * cout;
        for (int ci = 0; ci < cin; ++ci)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (co0 + j < cout) slab[(t * cin + ci) * cout + co0 + j] = red[(ci * 4 + j) * 192 + item];
    }
}

// ---------------------------------------------------------------- entries
#define SG_BY_COUT(LAUNCH)                                  \
    do {                                                    \
        if (cout % 8) { LAUNCH(64, false); }                \
        else switch (cout) {                                \
            case 8: LAUNCH(8, true); break;                 \
            case 16: LAUNCH(16, true); break;               \
            case 24: LAUNCH(24, true); break;               \
            case 32: LAUNCH(32, true); break;               \
            case 40: LAUNCH(40, true); break;               \
            case 48: LAUNCH(48, true); break;               \
            case 56: LAUNCH(56, true); break;               \
            default: LAUNCH(64, true); break;               \
        }                                                   \
    } while (0)

extern "C" int yr_conv3x3_forward(const float* x, int x_ld, const float* w, int B, int H, int W, int cin, int cout, int stride, int pad_top, int pad_left,
                                  int OH, int OW, float* y, int y_ld, void* stream) {
    YR_REQUIRE(x && w && y, "conv3x3_forward: null pointer");
    YR_REQUIRE(((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) % 4 == 0, "conv3x3_forward: x, w or y not 4-byte aligned");
    const int rc = sg_check("conv3x3_forward", B, H, W, cin, cout, stride, pad_top, pad_left, OH, OW, x_ld, y_ld);
    if (rc != YR_OK) return rc;
    const sg_geo d = {B, H, W, cin, cout, OH, OW, pad_top, pad_left, stride, x_ld, y_ld};
    const long long blocks = ((long long)B * OH * OW + 255) / 256;
    hipStream_t s = (hipStream_t)stream;
#define SG_LAUNCH(CT, EX) hipLaunchKernelGGL((sg_forward_kernel<CT, EX>), dim3((unsigned)blocks), dim3(256), 0, s, x, w, y, d)
    SG_BY_COUT(SG_LAUNCH);
#undef SG_LAUNCH
    YR_LAUNCH_CHECK();
    return YR_OK;
}

extern "C" int yr_conv3x3_dgrad(const float* dy, int dy_ld, const float* w, int B, int H, int W, int cin, int cout, int stride, int pad_top, int pad_left,
                                int OH, int OW, float* dx, int dx_ld, void* stream) {
    YR_REQUIRE(dy && w && dx, "conv3x3_dgrad: null pointer");
    YR_REQUIRE(((uintptr_t)dy | (uintptr_t)w | (uintptr_t)dx) % 4 == 0, "conv3x3_dgrad: dy, w or dx not 4-byte aligned");
    const int rc = sg_check("conv3x3_dgrad", B, H, W, cin, cout, stride, pad_top, pad_left, OH, OW, dx_ld, dy_ld);
    if (rc != YR_OK) return rc;
    const sg_geo d = {B, H, W, cin, cout, OH, OW, pad_top, pad_left, stride, dx_ld, dy_ld};
    const int QH = (H - 1 + pad_top) / stride + 1, QW = (W - 1 + pad_left) / stride + 1;      // cells that hold an input pixel
    const long long blocks = ((long long)B * QH * QW + 255) / 256;
    hipStream_t s = (hipStream_t)stream;
#define SG_LAUNCH(CT, EX)                                                                                                             \
    do {                                                                                                                              \
        if (stride == 1) hipLaunchKernelGGL((sg_dgrad_kernel<1, CT, EX>), dim3((unsigned)blocks), dim3(256), 0, s, dy, w, dx, d, QH, QW); \
        else hipLaunchKernelGGL((sg_dgrad_kernel<2, CT, EX>), dim3((unsigned)blocks), dim3(256), 0, s, dy, w, dx, d, QH, QW);             \
    } while (0)
    SG_BY_COUT(SG_LAUNCH);
#undef SG_LAUNCH
    YR_LAUNCH_CHECK();
    return YR_OK;
}

extern "C" int yr_conv3x3_wgrad(const float* x, int x_ld, const float* dy, int dy_ld, int B, int H, int W, int cin, int cout, int stride, int pad_top,
                                int pad_left, int OH, int OW, void* workspace, size_t workspace_bytes, float* dw, void* stream) {
    YR_REQUIRE(x && dy && workspace && dw, "conv3x3_wgrad: null pointer");
    YR_REQUIRE(((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dw) % 4 == 0, "conv3x3_wgrad: x, dy or dw not 4-byte aligned");
    const int rc = sg_check("conv3x3_wgrad", B, H, W, cin, cout, stride, pad_top, pad_left, OH, OW, x_ld, dy_ld);
    if (rc != YR_OK) return rc;
    const int wrc = tc_workspace_check("conv3x3_wgrad", workspace, workspace_bytes, yr_conv3x3_wgrad_workspace_bytes(B, OH, OW, cin, cout));
    if (wrc != YR_OK) return wrc;
    const int chunk = sg_chunk(B, OH, OW);
    const int nchunks = (int)(((long long)B * OH + chunk - 1) / chunk);
    const sg_geo d = {B, H, W, cin, cout, OH, OW, pad_top, pad_left, stride, x_ld, dy_ld};
    float* slabs = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sg_wgrad_partial_kernel, dim3(nchunks), dim3(256), 0, s, x, dy, slabs, d, chunk, sg_set_lanes(cout));
    YR_LAUNCH_CHECK();
    return yr_launch_slab_sum(slabs, nchunks, 9 * cin, cout, cout, dw, s);
}
