// Ground-truth boxes -> the y_true tensors YoloLoss reads, for a whole batch.  Replaces the per-image NumPy loop of reference
// code/yolo3/utils.py: preprocess_true_boxes :298-376 (restated on the host in yoloret_amd/yolo3/utils.py) and the dense upload
// of its result.  The bytes written are the host function's, quirks included:
//   * centre = floor((min + max) / 2) in float32 (:321, NumPy's // by 2), size = max - min in float32; the four relative values
//     are float64 quotients rounded once to float32 (NumPy divides a float32 array by an int32 array in float64 and rounds on
//     the store into the float32 array, :323-324);
//   * a row is valid when its float32 WIDTH is > 0 (:342);
//   * the best anchor is the first maximum over all nine anchors of the float32 IoU of the two centred boxes, in the operation
//     order of do_giou_calculate(anchor_box, bbox, mode='iou') (utils.py:9-40) with divide_no_nan; np.maximum / np.minimum hand a
//     NaN on and np.argmax takes the first NaN as the maximum (a NaN needs a size that overflowed to infinity);
//   * the r-th VALID row supplies the anchor, but row r of the unfiltered rows supplies the coordinates, the class and the cell
//     (:356-368);
//   * cell = floor(relative centre * grid) with the product formed in float64 (NumPy: float32 scalar times int32 scalar);
//   * the last row in index order that lands on a (scale, cell, slot) leaves its box there; class bits of all of them accumulate.
// Rows the host function cannot write (it raises, or a negative index wraps) write nothing here and are counted per image:
//   * a row with a non-finite value among its five is taken out BEFORE anything else: it neither counts as a row nor as a valid
//     row, the other rows are encoded as if it had not been in the list;
//   * a row whose truncated class is outside [0, C) or whose cell is outside the grid when its turn to be written comes.  The
//     range checks are made in floating point, phrased so that NaN fails them, before any conversion to an integer.
//
// Two launches on the caller's stream, no workspace, no host round trip:
//   1. enc_fill_kernel     zeroes the (up to) three tensors: grid-stride, 16-byte stores, scalar head and tail (a tensor starts on
//                          a 4-byte boundary at worst and its length is a multiple of 4 bytes, not of 16);
//   2. enc_scatter_kernel  one workgroup of 256 lanes per image, lane = row.  Ranks come from wave ballots and a prefix over the
//                          four waves; the (scale, cell, slot) key of every rank sits in LDS and a lane stores its box only if no
//                          higher rank holds the same key.  Flag and class-bit stores are the constant 1.0f from every lane that
//                          lands, so they need no order.  No atomics, no float accumulation: the same call gives the same bytes.
// The scatter is a launch of its own because it needs every zero written first.
#include "yr_common.h"

#define ENC_T YR_ENC_MAX_BOXES   // lanes per workgroup = rows per image
#define ENC_NO_KEY 0xffffffffu
#define ENC_FILL_BLOCKS 2048     // 256 CUs x 8 workgroups: the rest is walked grid-stride

struct EncArgs {
    const float* boxes;     // [B,T,5]
    int T;
    float ahw[9], ahh[9];   // anchors / 2 (:340): half width, half height
    int in_h, in_w, C, num_scales;
    float* y[3];
    int gh[3], gw[3];
    int32_t* skipped;
};

struct EncFill {
    float* p[3];
    size_t n[3];            // elements
};

__global__ __launch_bounds__(256) void enc_fill_kernel(EncFill a) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        float* p = a.p[l];
        const size_t n = a.n[l];
        if (p == nullptr) continue;
        size_t head = ((16 - ((uintptr_t)p & 15)) & 15) / 4;   // < 4 elements in front of the first 16-byte boundary
        if (head > n) head = n;
        const size_t nvec = (n - head) / 4, tail = head + nvec * 4;
        float4* v = reinterpret_cast<float4*>(p + head);
        for (size_t i = gid; i < nvec; i += stride) v[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gid < head) p[gid] = 0.0f;
        if (gid < n - tail) p[tail + gid] = 0.0f;              // < 4 elements behind the last whole float4
    }
}

__device__ __forceinline__ bool enc_finite(float v) { return fabsf(v) < __builtin_inff(); }   // false for NaN
// np.maximum / np.minimum: a NaN operand is the result
__device__ __forceinline__ float enc_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }
__device__ __forceinline__ float enc_min(float a, float b) { return a != a ? a : (b != b ? b : fminf(a, b)); }
// NumPy's float32 s // 2 (npy_divmod): floor(s / 2); the halving is exact except for the smallest negative denormal, which
// rounds to -0 where NumPy gives -1
__device__ __forceinline__ float enc_floordiv2(float s) {
    const float c = floorf(s * 0.5f);
    return (s < 0.0f && c == 0.0f) ? -1.0f : c;
}
// float32 array / int32 array: a float64 quotient, rounded on the store - NumPy's own two steps.  (A plain float32 divide gives the
// same bits whenever the divisor is exact in float32, i.e. up to 2^24; the entry takes any multiple of 32, and B x T x 4 float64
// divisions per call cost nothing next to the fill, so the literal form is kept for every size.)
__device__ __forceinline__ float enc_rel(float v, int d) { return (float)((double)v / (double)d); }

__global__ __launch_bounds__(ENC_T) void enc_scatter_kernel(EncArgs a) {
    __shared__ float sx[ENC_T], sy[ENC_T], sw[ENC_T], sh[ENC_T], sc[ENC_T];   // the finite rows, in order
    __shared__ int sanchor[ENC_T];                                            // best anchor, by rank among the valid rows
    __shared__ unsigned skey[ENC_T];                                          // (scale, cell, slot) a rank lands on
    __shared__ int wfin[ENC_T / 64], wval[ENC_T / 64], wskip[ENC_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const bool have = tid < a.T;
    float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f, r4 = 0.0f;
    if (have) {
        const float* t = a.boxes + ((size_t)b * a.T + tid) * 5;
        r0 = t[0]; r1 = t[1]; r2 = t[2]; r3 = t[3]; r4 = t[4];
    }
    const bool fin = have && enc_finite(r0) && enc_finite(r1) && enc_finite(r2) && enc_finite(r3) && enc_finite(r4);
    const float w = r2 - r0, h = r3 - r1;                                     // :322
    const bool valid = fin && w > 0.0f;                                       // :342
    // best anchor (:340-354): b1 = the anchor, b2 = the box, both centred on the origin
    int best = 0;
    if (valid) {
        const float bw = w / 2.0f, bh = h / 2.0f;
        const float barea = enc_max(0.0f, bw - (-bw)) * enc_max(0.0f, bh - (-bh));
        float best_iou = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float aw = a.ahw[k], ah = a.ahh[k];
            const float aarea = enc_max(0.0f, aw - (-aw)) * enc_max(0.0f, ah - (-ah));
            const float iw = enc_max(0.0f, enc_min(aw, bw) - enc_max(-aw, -bw));
            const float ih = enc_max(0.0f, enc_min(ah, bh) - enc_max(-ah, -bh));
            const float inter = iw * ih;
            const float uni = aarea + barea - inter;
            const float iou = uni != 0.0f ? inter / uni : 0.0f;               // divide_no_nan
            // np.argmax: the first maximum, a NaN being larger than everything
            if (k == 0 || (best_iou == best_iou && (iou > best_iou || iou != iou))) { best = k; best_iou = iou; }
        }
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long mfin = __ballot(fin), mval = __ballot(valid);
    if (lane == 0) { wfin[wave] = __popcll(mfin); wval[wave] = __popcll(mval); }
    __syncthreads();
    int fpos = __popcll(mfin & below), rank = __popcll(mval & below), nvalid = 0;
#pragma unroll
    for (int k = 0; k < ENC_T / 64; ++k) {
        if (k < wave) { fpos += wfin[k]; rank += wval[k]; }
        nvalid += wval[k];
    }
    if (fin) {   // :323-324, after :321
        sx[fpos] = enc_rel(enc_floordiv2(r0 + r2), a.in_w);
        sy[fpos] = enc_rel(enc_floordiv2(r1 + r3), a.in_h);
        sw[fpos] = enc_rel(w, a.in_w);
        sh[fpos] = enc_rel(h, a.in_h);
        sc[fpos] = r4;
    }
    if (valid) sanchor[rank] = best;
    __syncthreads();

    // lane r now plays rank r: the anchor of the r-th valid row with row r of the finite rows (r < nvalid <= their number)
    bool hit = false, skip = false;
    unsigned key = ENC_NO_KEY;
    float x = 0.0f, y = 0.0f, bwr = 0.0f, bhr = 0.0f;
    int cls = 0, slot = 0, l = -1, gh = 1, gw = 1, cell = 0;
    if (tid < nvalid) {
        const int n = sanchor[tid];
        l = (2 - n / 3) - (3 - a.num_scales);     // anchor_mask[-num_scales:] (:318): anchors of a scale that is left out land nowhere
        if (l >= 0) {
            slot = n % 3;
            gh = l == 0 ? a.gh[0] : (l == 1 ? a.gh[1] : a.gh[2]);
            gw = l == 0 ? a.gw[0] : (l == 1 ? a.gw[1] : a.gw[2]);
            x = sx[tid]; y = sy[tid]; bwr = sw[tid]; bhr = sh[tid];
            const float c = sc[tid];
            const double col = floor((double)x * (double)gw), row = floor((double)y * (double)gh);   // :359-362
            const float ct = truncf(c);             // int(): toward zero; the range is checked on the truncated value (with C = 0
            //                                          a class in (-1, 0) truncates to 0, which is no class bit either)
            hit = col >= 0.0 && col < (double)gw && row >= 0.0 && row < (double)gh && ct >= 0.0f && ct < (float)a.C;
            skip = !hit;
            if (hit) {
                cls = (int)ct;
                cell = (int)row * gw + (int)col;
                // int arithmetic: an output holds at most 2^31 elements of 5 + C >= 5 floats, so cell * 3 + slot < 2^31 / 5 < 2^29
                key = ((unsigned)l << 29) | (unsigned)(cell * 3 + slot);
            }
        }
    }
    skey[tid] = key;
    // two sets of rows, counted apart: `skip` is about the finite row this lane plays as a rank, `have && !fin` about the lane's own row
    const int nskip = __popcll(__ballot(skip)) + __popcll(__ballot(have && !fin));
    if (lane == 0) wskip[wave] = nskip;
    __syncthreads();
    if (tid == 0 && a.skipped != nullptr) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < ENC_T / 64; ++k) s += wskip[k];
        a.skipped[b] = s;
    }
    if (!hit) return;
    bool last = true;
    for (int r = tid + 1; r < nvalid; ++r) last = last && skey[r] != key;
    float* out = l == 0 ? a.y[0] : (l == 1 ? a.y[1] : a.y[2]);
    float* e = out + (((size_t)b * gh * gw + cell) * 3 + slot) * (size_t)(5 + a.C);
    if (last) { e[0] = x; e[1] = y; e[2] = bwr; e[3] = bhr; }   // :366
    e[4] = 1.0f;                                                // :367
    e[5 + cls] = 1.0f;                                          // :368
}

extern "C" int yr_encode_labels(const float* true_boxes, int batch, int max_boxes, int in_h, int in_w, const float* anchors_host,
                                int num_classes, int num_scales, float* y1, float* y2, float* y3, int32_t* skipped, void* stream) {
    YR_REQUIRE(true_boxes && anchors_host, "encode_labels: null pointer");
    YR_REQUIRE(batch > 0, "encode_labels: batch must be positive, not %d", batch);
    YR_REQUIRE(max_boxes >= 1 && max_boxes <= YR_ENC_MAX_BOXES, "encode_labels: max_boxes must be 1..%d, not %d", YR_ENC_MAX_BOXES, max_boxes);
    YR_REQUIRE(num_scales >= 1 && num_scales <= 3, "encode_labels: num_scales must be 1..3, not %d", num_scales);
    YR_REQUIRE(num_classes >= 0, "encode_labels: num_classes must not be negative (%d)", num_classes);
    YR_REQUIRE(in_h > 0 && in_w > 0 && in_h % 32 == 0 && in_w % 32 == 0, "encode_labels: input %dx%d, positive multiples of 32 expected", in_h, in_w);
    float* ys[3] = {y1, y2, y3};
    EncArgs a;
    EncFill f;
    size_t nvec = 0;
    for (int l = 0; l < 3; ++l) {
        const bool used = l < num_scales;
        YR_REQUIRE(!used || ys[l], "encode_labels: output %d of %d scales is null", l + 1, num_scales);
        a.gh[l] = in_h / (32 >> l); a.gw[l] = in_w / (32 >> l);
        const long long n = (long long)batch * a.gh[l] * a.gw[l] * 3 * (5ll + num_classes);
        YR_REQUIRE(!used || n <= (1ll << 31), "encode_labels: output %d has more than 2^31 elements", l + 1);
        a.y[l] = used ? ys[l] : nullptr;
        f.p[l] = a.y[l];
        f.n[l] = used ? (size_t)n : 0;
        nvec += f.n[l] / 4 + 1;
    }
    a.boxes = true_boxes; a.T = max_boxes;
    for (int k = 0; k < 9; ++k) {
        a.ahw[k] = anchors_host[k * 2] / 2.0f;
        a.ahh[k] = anchors_host[k * 2 + 1] / 2.0f;
    }
    a.in_h = in_h; a.in_w = in_w; a.C = num_classes; a.num_scales = num_scales;
    a.skipped = skipped;
    hipStream_t s = (hipStream_t)stream;
    const size_t blocks = (nvec + 255) / 256;
    hipLaunchKernelGGL(enc_fill_kernel, dim3((unsigned)(blocks < ENC_FILL_BLOCKS ? blocks : ENC_FILL_BLOCKS)), dim3(256), 0, s, f);
    YR_LAUNCH_CHECK();
    hipLaunchKernelGGL(enc_scatter_kernel, dim3(batch), dim3(ENC_T), 0, s, a);
    YR_LAUNCH_CHECK();
    return YR_OK;
}
