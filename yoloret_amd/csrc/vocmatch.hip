// VOC matching of packed detections to ground truth, per image, on the device.  Replaces the greedy loop of the reference's
// MAPCallback.calculate_aps (code/yolo3/map.py:157-215): detections of a class in score order, each claiming its best-overlapping
// ground-truth box of that class in the same image if the IoU exceeds the threshold and the box is not claimed yet.
//
// Why one workgroup per image gives the data set's verdicts: a detection can only claim a box of its own image and class, so the
// reference's pass over ALL detections of a class in global score order visits the detections of one (image, class) group in that
// group's score order, and no other detection touches the group's claims.
//
// Bit-exactness with the host evaluator (yolo3/map.py: evaluate_detections):
//   * order inside a group: score descending, compared as float32 VALUES (-0 == +0), ties by lower row index (its stable sort);
//   * IoU with the VOC +1 convention in float64, in the host's operation order; the library is built with -ffp-contract=off and
//     -fno-fast-math, so add / multiply / divide are the correctly rounded IEEE operations NumPy performs;
//   * best box = maximum IoU over the ground truth of the class, ties to the lowest index (np.argmax), chosen BEFORE the claim
//     check: a detection whose best box is taken is a false positive even if an equally good free box exists;
//   * strict threshold: ov > iou_thr.
// Contract: finite scores and coordinates, max >= min on both axes of every box (then union >= 1 and no NaN arises).
//
// One launch, one workgroup of 256 lanes per image, no workspace, no atomics on global memory, no host synchronisation:
//   1. stage a 64-bit sort key per valid row (class << 32 | descending-score key; rows with a class outside [0, C) get a key above
//      every valid one) and the image's ground truth into LDS; rows that get no verdict are written -1 here;
//   2. npos; the rank of every row in (class, score descending, row) order by counting over LDS broadcasts (O(n^2), n <= 4096),
//      scattered into a sorted row list;
//   3. positions of that list where the class changes are appended to a segment list (LDS counter: the order of the list does not
//      matter, every segment is processed by exactly one wave);
//   4. each wave takes segments round-robin.  The boxes of up to 64 detections are fetched at once, one per lane, and broadcast
//      in rank order; per detection the lanes evaluate 64 ground-truth rows at a time, a butterfly gives the argmax over
//      (ov, lowest index), lane 0 writes the verdict.  Claim bits stay in the wave's registers (bit k of lane l: row 64k + l).
// Rows at or beyond det_count[b] / gt_count[b] are never read.
#include "yr_common.h"
#include <limits.h>

#define VOC_T 256
#define VOC_WAVES (VOC_T / 64)
#define VOC_CHUNKS (YR_VOC_MAX_GT / 64)
#define VOC_NO_CLASS 0xffffffffu     // class word of a row that gets no verdict; above every valid class (< 2^31)

static_assert(YR_VOC_MAX_ROWS <= 65536, "row indices are kept as 16-bit words");
static_assert(VOC_CHUNKS <= 32, "claim bits of a lane are one 32-bit word");

struct VocArgs {
    const int32_t* det;         // [B,rows,6]
    const int32_t* det_count;   // [B]
    const float* gt;            // [B,max_gt,5] (xmin, ymin, xmax, ymax, label)
    const int32_t* gt_count;    // [B]
    int rows, C, max_gt;
    double thr;
    int32_t* flags;             // [B,rows]
    int32_t* npos;              // [B,C]
};

// ascending in this key = descending in the score's float32 value
__device__ __forceinline__ unsigned voc_score_key(float s) {
    unsigned u = __float_as_uint(s == 0.0f ? 0.0f : s);      // -0 and +0 are one value
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);          // ascending in s
    return ~u;
}

__device__ __forceinline__ unsigned voc_class_of(unsigned long long key) { return (unsigned)(key >> 32); }

__global__ __launch_bounds__(VOC_T) void voc_match_kernel(VocArgs a) {
    __shared__ unsigned long long s_key[YR_VOC_MAX_ROWS];
    __shared__ float s_gt[YR_VOC_MAX_GT * 5];
    __shared__ unsigned short s_order[YR_VOC_MAX_ROWS];     // valid rows in (class, score descending, row) order
    __shared__ unsigned short s_seg[YR_VOC_MAX_ROWS];       // first position of every class segment of s_order, in any order
    __shared__ int s_nvalid, s_nseg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    const int n = min(max(a.det_count[b], 0), a.rows);
    const int ngt = min(max(a.gt_count[b], 0), a.max_gt);
    const int32_t* det = a.det + b * (size_t)a.rows * 6;
    int32_t* flags = a.flags + b * (size_t)a.rows;
    if (tid == 0) { s_nvalid = 0; s_nseg = 0; }
    __syncthreads();

    // ---- 1. stage
    int nval = 0;
    for (int i = tid; i < a.rows; i += VOC_T) {
        bool valid = false;
        if (i < n) {
            const int c = det[i * 6 + 5];
            valid = c >= 0 && c < a.C;
            s_key[i] = ((unsigned long long)(valid ? (unsigned)c : VOC_NO_CLASS) << 32) | voc_score_key(__int_as_float(det[i * 6 + 4]));
        }
        if (!valid) flags[i] = -1;
        nval += valid ? 1 : 0;
    }
    if (nval) atomicAdd(&s_nvalid, nval);
    if (ngt) {
        const float* gt = a.gt + b * (size_t)a.max_gt * 5;
        for (int k = tid; k < ngt * 5; k += VOC_T) s_gt[k] = gt[k];
    }
    __syncthreads();

    // ---- 2. npos, then rank and scatter
    for (int c = tid; c < a.C; c += VOC_T) {
        const double cd = (double)c;
        int cnt = 0;
        for (int g = 0; g < ngt; ++g) cnt += ((double)s_gt[g * 5 + 4] == cd) ? 1 : 0;     // the host's boxes[:, 4] == cls
        a.npos[b * (size_t)a.C + c] = cnt;
    }
    for (int base = 0; base < n; base += VOC_T * 4) {
        unsigned long long k[4];
        int row[4], pos[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            row[r] = base + r * VOC_T + tid;
            k[r] = row[r] < n ? s_key[row[r]] : ~0ull;
            pos[r] = 0;
        }
        for (int j = 0; j < n; ++j) {
            const unsigned long long kj = s_key[j];      // one address for the whole wave: a broadcast
#pragma unroll
            for (int r = 0; r < 4; ++r) pos[r] += (kj < k[r] || (kj == k[r] && j < row[r])) ? 1 : 0;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (row[r] < n && voc_class_of(k[r]) != VOC_NO_CLASS) s_order[pos[r]] = (unsigned short)row[r];   // pos < s_nvalid: rows without a class sort last
    }
    __syncthreads();

    // ---- 3. class segments
    const int nv = s_nvalid;
    for (int p = tid; p < nv; p += VOC_T)
        if (p == 0 || voc_class_of(s_key[s_order[p - 1]]) != voc_class_of(s_key[s_order[p]])) s_seg[atomicAdd(&s_nseg, 1)] = (unsigned short)p;
    __syncthreads();

    // ---- 4. greedy matching, one wave per class segment.  Everything that steers control flow below is wave-uniform.
    const int nseg = s_nseg;
    const int nchunks = (ngt + 63) >> 6;
    for (int s = wave; s < nseg; s += VOC_WAVES) {
        const int start = s_seg[s];
        const unsigned c = voc_class_of(s_key[s_order[start]]);
        const double cd = (double)c;
        unsigned mine = 0, anyc = 0;      // bit k: ground-truth row 64k + lane has this class / some row of chunk k has it
        for (int k = 0; k < nchunks; ++k) {
            const int g = k * 64 + lane;
            const bool m = g < ngt && (double)s_gt[g * 5 + 4] == cd;
            mine |= (m ? 1u : 0u) << k;
            anyc |= (__ballot(m) ? 1u : 0u) << k;
        }
        unsigned claimed = 0;
        for (int q = start;; q += 64) {
            const int p = q + lane;
            int row = 0;
            bool in = false;
            if (p < nv) {
                row = s_order[p];
                in = voc_class_of(s_key[row]) == c;
            }
            const int cnt = __popcll(__ballot(in));      // the segment is contiguous: the lanes inside it are lanes 0 .. cnt-1
            int y1 = 0, x1 = 0, y2 = 0, x2 = 0;
            if (in) {
                const int32_t* d = det + row * 6;
                y1 = d[0]; x1 = d[1]; y2 = d[2]; x2 = d[3];
            }
            for (int k = 0; k < cnt; ++k) {
                const int r = __shfl(row, k);
                double best = -1.0;           // every IoU is >= 0
                int bi = INT_MAX;
                if (anyc) {
                    const double bx1 = (double)__shfl(x1, k), by1 = (double)__shfl(y1, k), bx2 = (double)__shfl(x2, k), by2 = (double)__shfl(y2, k);
                    const double area = (bx2 - bx1 + 1.0) * (by2 - by1 + 1.0);
                    for (int ch = 0; ch < nchunks; ++ch) {
                        if (!((mine >> ch) & 1u)) continue;
                        const int g = ch * 64 + lane;
                        const double gx1 = (double)s_gt[g * 5], gy1 = (double)s_gt[g * 5 + 1], gx2 = (double)s_gt[g * 5 + 2], gy2 = (double)s_gt[g * 5 + 3];
                        const double iw = fmax(fmin(gx2, bx2) - fmax(gx1, bx1) + 1.0, 0.0);
                        const double ih = fmax(fmin(gy2, by2) - fmax(gy1, by1) + 1.0, 0.0);
                        const double inter = iw * ih;
                        const double uni = area + (gx2 - gx1 + 1.0) * (gy2 - gy1 + 1.0) - inter;
                        const double ov = inter / uni;
                        if (ov > best) { best = ov; bi = g; }      // strict: a tie keeps the lower index
                    }
#pragma unroll
                    for (int off = 32; off; off >>= 1) {
                        const double ob = __shfl_xor(best, off);
                        const int oi = __shfl_xor(bi, off);
                        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
                    }
                }
                bool tp = false;
                if (bi != INT_MAX && best > a.thr) {
                    const unsigned cl = __shfl(claimed, bi & 63);
                    tp = !((cl >> (bi >> 6)) & 1u);
                    if (tp && lane == (bi & 63)) claimed |= 1u << (bi >> 6);
                }
                if (lane == 0) flags[r] = tp ? 1 : 0;
            }
            if (cnt < 64) break;
        }
    }
}

extern "C" int yr_voc_match(const int32_t* det, const int32_t* det_count, int batch, int rows, int num_classes,
                            const float* gt, const int32_t* gt_count, int max_gt, double iou_thr,
                            int32_t* flags, int32_t* npos, void* stream) {
    YR_REQUIRE(det && det_count && gt_count && flags && npos, "voc_match: null pointer");
    YR_REQUIRE(batch > 0, "voc_match: batch must be positive, not %d", batch);
    YR_REQUIRE(rows >= 1 && rows <= YR_VOC_MAX_ROWS, "voc_match: %d rows per image, 1..%d supported", rows, YR_VOC_MAX_ROWS);
    YR_REQUIRE(max_gt >= 0 && max_gt <= YR_VOC_MAX_GT, "voc_match: %d ground-truth rows per image, 0..%d supported", max_gt, YR_VOC_MAX_GT);
    YR_REQUIRE(gt || max_gt == 0, "voc_match: null ground truth with max_gt = %d", max_gt);
    YR_REQUIRE(num_classes >= 1, "voc_match: num_classes must be at least 1, not %d", num_classes);
    VocArgs a;
    a.det = det; a.det_count = det_count; a.gt = gt; a.gt_count = gt_count;
    a.rows = rows; a.C = num_classes; a.max_gt = max_gt;
    a.thr = iou_thr;
    a.flags = flags; a.npos = npos;
    hipLaunchKernelGGL(voc_match_kernel, dim3(batch), dim3(VOC_T), 0, (hipStream_t)stream, a);
    YR_LAUNCH_CHECK();
    return YR_OK;
}
