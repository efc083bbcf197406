// YoloLoss forward, GIOU branch, for ONE scale.  Replaces the TF graph behind reference code/yolo3/model.py: YoloLoss.call
// :607-671 with yolo_head(calc_loss=True) :344-369 and do_giou_calculate (code/yolo3/utils.py:9-53): the forward (yr_yolo_loss) and
// the gradient of that scalar with respect to the logits (yr_yolo_loss_grad, rules below); no backward through the network.
//
// What is reproduced, quirks included:
//   * masked_true_box (:643) is gathered over the WHOLE batch of the call: a prediction of image 0 is compared with the labelled
//     boxes of every image.  That is what the reference computes, so that is what is computed here.
//   * with no labelled box in the call, the maximum over the empty set is below every threshold: every cell is ignored (:648-649).
//   * the true boxes are clipped to [0,1] (:640), the predicted ones are not.
// Per-element arithmetic is float32 in the reference's operation order with no FMA contraction (library built with
// -ffp-contract=off); exp through yr_expf and sigmoid through yr_sigmoid, so pred_xy / pred_wh are bit-identical to what
// yolo_head_kernel (postprocess.hip) writes; log1p is the device library's float32 log1pf.  The sums are float64 in a FIXED order
// (lane -> wave butterfly -> waves in index order -> one row per workgroup -> rows in a fixed order) and rounded to float32 once:
// no float atomics and no in-launch hand-off between workgroups, so a call is bit-reproducible whatever the arrival order.
// Non-finite logits or labels are outside the contract (a NaN would make the maximum depend on the order of the box list).
//
// Three launches on the caller's stream, no host round trip:
//   1. loss_compact_kernel  appends the clipped box of every object cell (y_true[..., 4] != 0) to a list in the workspace;
//   2. loss_main_kernel     one lane per prediction: decode, best IoU over the list (LDS-resident chunks), the lane's terms;
//   3. loss_final_kernel    sums the workgroup rows, divides by B, writes {loss, giou, conf, class, ignore_sum}.
// Workspace: [0,256) header (word 0: the number of listed boxes), then the list (float4 per box, room for every cell), then one
// LossRow per workgroup of the main pass.  Nothing in it is read before this call has written it.
//
// The gradient (yr_yolo_loss_grad): dfeats = upstream * d loss / d feats, [B,gh,gw,A,5+C] float32, m = B, in the same three launches
// (loss_main_kernel<true>), so out5 holds the bits yr_yolo_loss writes.  The rules are what TensorFlow's autodiff gives for
// model.py:607-671; like the rest of the oracle they are UNPINNED BY THE REFERENCE (no TensorFlow where this is tested) and pinned
// by hand-derived answers and finite differences of the float64 restatement (tests/lossgrad_ref.py, tests/test_lossgrad_host.py).
// Pinned on the device (tests/test_gpu_lossgrad_edges.py, against that restatement with every Maximum / Minimum as a select, which
// makes it valid AT ties): the tie rules below at all 13 x 13 interval relations of a label to its prediction and at zero-size
// labels; the strict threshold at an IoU of exactly 0.5; box lists of one chunk exactly, one box more, two and three chunks; rows
// of 5 to 305 floats (C = 0 .. 300: LOSS_T / row == 0 and LOSS_T % row == 0 included); A from 1 to 8; totals below and equal to
// LOSS_T; object flags other than 1.  Outside the contract: non-finite inputs, and logits beyond yr_expf's clamp (last rule).
//   * ignore_mask (:649) is the result of a comparison: a constant.  best_iou (:644-648) contributes nothing.
//   * channel 4:    ((om + (1 - om) * ignore) * (sigmoid(x4) - om)) / m          [d sce(z, x) / dx = sigmoid(x) - z; :653-657, :663]
//   * channels 5..: (om * (sigmoid(x_c) - t_c)) / m, exactly 0 where om == 0     [:658-662]
//   * channels 0-3: (-om / m) * d giou / d(pred box) (:666-668), chained through loss_box (centre and size -> corners, :631-633)
//     and the decode (:363-366): d px / d x0 = s (1 - s) / gw with s = sigmoid(x0), d py / d x1 likewise with gh,
//     d pw / d x2 = pw, d ph / d x3 = ph.  The true box is a constant (its clip to [0,1] never enters).  0 where om == 0.
//   * kinks: tf.maximum(a, b) sends the gradient to a where a >= b, else to b; tf.minimum(a, b) to a where a <= b;
//     tf.maximum(zero, v) has zero as its FIRST operand, so v receives it only where v > 0.  b1 is the prediction throughout
//     do_giou_calculate, so every tie goes to the prediction.  divide_no_nan has zero gradient where the denominator is 0.
//   * per corner k of the prediction, with u = union, i = intersection, e = enclosing area and d_k their derivatives (products of
//     the indicator above and the other side's length):  d_k giou = (u d_k i - i d_k u) / u^2 + (e d_k u - u d_k e) / e^2,
//     d_k u = d_k area1 - d_k i.  The quotient-rule grouping keeps the difference of two equal products exact (a prediction that
//     encloses its label: e d_k u == u d_k e), where the term-by-term chain would cancel two rounded quotients.
//   * yr_expf clamps its argument to [-87, 88]; the gradient takes pw, ph as the forward computed them (logits beyond the clamp
//     are outside any trained range).
// Per-element arithmetic is float32, pred_* are the forward's values; `upstream` (one float on the device, null = 1) multiplies each
// finished element as the last operation, so a power of two scales the result exactly.  EVERY element of dfeats is written, zeros
// included.  Two phases inside the workgroup: one lane per prediction leaves the four box gradients, the confidence gradient and
// om in LDS; then the workgroup walks its contiguous 256 x (5+C) floats one element per lane (coalesced dword stores) and reads
// class logits and class bits only in rows with om != 0.  No atomics beyond the box-list counter: bit-reproducible.
#include "yr_common.h"

#define LOSS_T 256          // lanes per workgroup = boxes per LDS chunk
#define LOSS_HEADER 256     // bytes in front of the box list

struct LossRow {
    double giou, conf, cls;
    long long ignore;
};

struct LossArgs {
    const float* feats;     // [B,gh,gw,A,5+C] logits
    const float* y_true;    // same shape: (x, y, w, h, object, class bits)
    float anchors[8][2];
    int gh, gw, A, C, in_h, in_w, batch;
    int total;              // B*gh*gw*A
    float ignore_thresh;
    unsigned* count;        // listed boxes
    float4* list;           // (y_min, x_min, y_max, x_max), clipped
    LossRow* rows;
    int nrows;
    float* out5;
    float* dfeats;          // gradient form only: [B,gh,gw,A,5+C]
    const float* upstream;  // gradient form only: one float on the device, or null for 1
};

// model.py:631-633 / :637-639: (y_min, x_min, y_max, x_max) from centre and size
__device__ __forceinline__ float4 loss_box(float x, float y, float w, float h) {
    const float hw = w / 2.0f, hh = h / 2.0f;
    return make_float4(y - hh, x - hw, y + hh, x + hw);
}

// tf.clip_by_value(v, 0, 1)
__device__ __forceinline__ float loss_clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// utils.py:24-29
__device__ __forceinline__ float loss_area(float4 b) { return fmaxf(0.0f, b.w - b.y) * fmaxf(0.0f, b.z - b.x); }

// tf.math.divide_no_nan: a zero denominator gives 0
__device__ __forceinline__ float loss_div_no_nan(float a, float b) { return b == 0.0f ? 0.0f : a / b; }

// tf.nn.sigmoid_cross_entropy_with_logits(labels=z, logits=x) = (max(x,0) - x*z) + log1p(exp(-|x|))
__device__ __forceinline__ float loss_sce(float z, float x) { return (fmaxf(x, 0.0f) - x * z) + log1pf(yr_expf(-fabsf(x))); }

// d giou(pb, tb) / d pb (utils.py:24-53 differentiated, b1 = pb the prediction, b2 = tb a constant) in the grouping of the header
// comment.  The forward values are formed by the forward's expressions.  -> (d/d y_min, d/d x_min, d/d y_max, d/d x_max)
__device__ __forceinline__ float4 loss_giou_grad(float4 pb, float4 tb) {
    const float w1r = pb.w - pb.y, h1r = pb.z - pb.x;
    const float w1 = fmaxf(0.0f, w1r), h1 = fmaxf(0.0f, h1r);
    const float parea = w1 * h1, tarea = loss_area(tb);
    const float iwr = fminf(pb.w, tb.w) - fmaxf(pb.y, tb.y), ihr = fminf(pb.z, tb.z) - fmaxf(pb.x, tb.x);
    const float iw = fmaxf(0.0f, iwr), ih = fmaxf(0.0f, ihr);
    const float inter = iw * ih;
    const float uni = parea + tarea - inter;
    const float ewr = fmaxf(pb.w, tb.w) - fminf(pb.y, tb.y), ehr = fmaxf(pb.z, tb.z) - fminf(pb.x, tb.x);
    const float ew = fmaxf(0.0f, ewr), eh = fmaxf(0.0f, ehr);
    const float earea = ew * eh;
    const float uu = uni * uni, ee = earea * earea;
    // one corner: ds, di, de = d(own side) / d corner of the prediction, the intersection and the enclosing box (-1, 0 or 1);
    // os, oi, oe = the lengths of the other side
    auto corner = [&](float ds, float di, float de, float os, float oi, float oe) {
        const float d_area = ds * os, d_inter = di * oi, d_earea = de * oe;
        const float d_uni = d_area - d_inter;
        const float a = uni == 0.0f ? 0.0f : (uni * d_inter - inter * d_uni) / uu;
        const float b = earea == 0.0f ? 0.0f : (earea * d_uni - uni * d_earea) / ee;
        return a + b;
    };
    const float wp = w1r > 0.0f ? 1.0f : 0.0f, hp = h1r > 0.0f ? 1.0f : 0.0f;
    const bool iwp = iwr > 0.0f, ihp = ihr > 0.0f, ewp = ewr > 0.0f, ehp = ehr > 0.0f;
    float4 g;
    g.x = corner(-hp, (ihp && pb.x >= tb.x) ? -1.0f : 0.0f, (ehp && pb.x <= tb.x) ? -1.0f : 0.0f, w1, iw, ew);   // y_min
    g.y = corner(-wp, (iwp && pb.y >= tb.y) ? -1.0f : 0.0f, (ewp && pb.y <= tb.y) ? -1.0f : 0.0f, h1, ih, eh);   // x_min
    g.z = corner(hp, (ihp && pb.z <= tb.z) ? 1.0f : 0.0f, (ehp && pb.z >= tb.z) ? 1.0f : 0.0f, w1, iw, ew);      // y_max
    g.w = corner(wp, (iwp && pb.w <= tb.w) ? 1.0f : 0.0f, (ewp && pb.w >= tb.w) ? 1.0f : 0.0f, h1, ih, eh);      // x_max
    return g;
}

__global__ __launch_bounds__(LOSS_T) void loss_compact_kernel(LossArgs a) {
    const int gid = (int)blockIdx.x * LOSS_T + (int)threadIdx.x;
    const int lane = threadIdx.x & 63;
    const float* t = a.y_true + (size_t)min(gid, a.total - 1) * (a.C + 5);
    const bool obj = gid < a.total && t[4] != 0.0f;
    const unsigned long long mask = __ballot(obj);
    if (!mask) return;   // wave-uniform
    // One atomic per wave.  The list's order is arrival order, which is harmless BECAUSE THE ONLY THING COMPUTED FROM THE LIST IS A
    // MAXIMUM (best_iou, :648): a maximum of finite floats does not depend on the order of its operands.
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(a.count, (unsigned)__popcll(mask));
    base = __shfl(base, 0);
    if (obj) {
        float4 b = loss_box(t[0], t[1], t[2], t[3]);
        b = make_float4(loss_clip01(b.x), loss_clip01(b.y), loss_clip01(b.z), loss_clip01(b.w));   // :640
        a.list[base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull))] = b;   // < total: at most one entry per cell
    }
}

// GRAD = false is the forward of yr_yolo_loss; GRAD = true adds the gradient without touching an operation of the forward.
template <bool GRAD>
__global__ __launch_bounds__(LOSS_T) void loss_main_kernel(LossArgs a) {
    __shared__ float4 sbox[LOSS_T];
    __shared__ float sarea[LOSS_T];
    __shared__ LossRow swave[LOSS_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gid = (int)blockIdx.x * LOSS_T + tid;
    const bool valid = gid < a.total;
    const int row = a.C + 5;
    const size_t off = (size_t)min(gid, a.total - 1) * row;
    const float* t = a.feats + off;
    const float* yt = a.y_true + off;
    const int an = gid % a.A;
    const int cell = gid / a.A;
    const int w = cell % a.gw, h = (cell / a.gw) % a.gh;
    // yolo_head (model.py:363-366), the expressions of yolo_head_kernel
    const float px = (yr_sigmoid(t[0]) + (float)w) / (float)a.gw;
    const float py = (yr_sigmoid(t[1]) + (float)h) / (float)a.gh;
    const float pw = yr_expf(t[2]) * a.anchors[an][0] / (float)a.in_w;
    const float ph = yr_expf(t[3]) * a.anchors[an][1] / (float)a.in_h;
    const float4 pb = loss_box(px, py, pw, ph);
    const float parea = loss_area(pb);

    // best_iou (:644-648) over the listed boxes of the whole call.  A chunk of the list sits in LDS; every lane reads the same
    // address (a broadcast).  The maximum over an empty list is -inf: every cell is then ignored.
    const unsigned n = *a.count;
    float best = -__builtin_inff();
    for (unsigned c0 = 0; c0 < n; c0 += LOSS_T) {
        __syncthreads();
        if (c0 + tid < n) {
            const float4 b = a.list[c0 + tid];
            sbox[tid] = b;
            sarea[tid] = loss_area(b);
        }
        __syncthreads();
        const int m = (int)min((unsigned)LOSS_T, n - c0);
        for (int k = 0; k < m; ++k) {
            const float4 tb = sbox[k];
            // utils.py:31-40
            const float iw = fmaxf(0.0f, fminf(pb.w, tb.w) - fmaxf(pb.y, tb.y));
            const float ih = fmaxf(0.0f, fminf(pb.z, tb.z) - fmaxf(pb.x, tb.x));
            const float inter = iw * ih;
            // a zero intersection gives 0 / union = 0, or 0 by divide_no_nan: the division is only needed where boxes meet
            float iou = 0.0f;
            if (inter > 0.0f) iou = loss_div_no_nan(inter, parea + sarea[k] - inter);
            best = fmaxf(best, iou);
        }
    }
    const float ignore = best < a.ignore_thresh ? 1.0f : 0.0f;   // :649, strict

    double giou_t = 0.0, conf_t = 0.0, cls_t = 0.0;
    long long ign_t = 0;
    float gx0 = 0.0f, gx1 = 0.0f, gx2 = 0.0f, gx3 = 0.0f, gconf = 0.0f, gom = 0.0f;   // GRAD: this prediction's row, channels 0-4, and om
    if (valid) {
        const float om = yt[4];
        const float ce = loss_sce(om, t[4]);
        conf_t = (double)(om * ce + (1.0f - om) * ce * ignore);   // :653-657
        ign_t = best < a.ignore_thresh ? 1 : 0;                   // :671 counts object cells too
        if (om != 0.0f) {   // other cells contribute exactly 0 to the class and GIoU terms
            for (int c = 0; c < a.C; ++c) cls_t += (double)(om * loss_sce(yt[5 + c], t[5 + c]));   // :658-659
            float4 tb = loss_box(yt[0], yt[1], yt[2], yt[3]);
            tb = make_float4(loss_clip01(tb.x), loss_clip01(tb.y), loss_clip01(tb.z), loss_clip01(tb.w));
            // utils.py:24-53 with b1 = pred_box, b2 = true_box
            const float tarea = loss_area(tb);
            const float iw = fmaxf(0.0f, fminf(pb.w, tb.w) - fmaxf(pb.y, tb.y));
            const float ih = fmaxf(0.0f, fminf(pb.z, tb.z) - fmaxf(pb.x, tb.x));
            const float inter = iw * ih;
            const float uni = parea + tarea - inter;
            const float iou = loss_div_no_nan(inter, uni);
            const float ew = fmaxf(0.0f, fmaxf(pb.w, tb.w) - fminf(pb.y, tb.y));
            const float eh = fmaxf(0.0f, fmaxf(pb.z, tb.z) - fminf(pb.x, tb.x));
            const float earea = ew * eh;
            const float giou = iou - loss_div_no_nan(earea - uni, earea);
            giou_t = (double)(om * (1.0f - giou));   // :667
            if constexpr (GRAD) {
                const float4 g = loss_giou_grad(pb, tb);
                // corners -> centre and size (:631-633), then the decode (:363-366)
                const float gpx = g.y + g.w, gpy = g.x + g.z, gpw = (g.w - g.y) / 2.0f, gph = (g.z - g.x) / 2.0f;
                const float sx = yr_sigmoid(t[0]), sy = yr_sigmoid(t[1]);
                const float sc = -om / (float)a.batch;
                gx0 = sc * (gpx * (sx * (1.0f - sx) / (float)a.gw));
                gx1 = sc * (gpy * (sy * (1.0f - sy) / (float)a.gh));
                gx2 = sc * (gpw * pw);
                gx3 = sc * (gph * ph);
            }
        }
        if constexpr (GRAD) {
            gconf = ((om + (1.0f - om) * ignore) * (yr_sigmoid(t[4]) - om)) / (float)a.batch;
            gom = om;
        }
    }
    __shared__ float sgrad[GRAD ? 6 : 1][LOSS_T];
    if constexpr (GRAD) {   // (read after the barrier below)
        sgrad[0][tid] = gx0; sgrad[1][tid] = gx1; sgrad[2][tid] = gx2; sgrad[3][tid] = gx3; sgrad[4][tid] = gconf; sgrad[5][tid] = gom;
    }
    // wave butterfly, then the waves in index order: a fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        giou_t += __shfl_xor(giou_t, o);
        conf_t += __shfl_xor(conf_t, o);
        cls_t += __shfl_xor(cls_t, o);
        ign_t += __shfl_xor(ign_t, o);
    }
    if (lane == 0) { swave[wave].giou = giou_t; swave[wave].conf = conf_t; swave[wave].cls = cls_t; swave[wave].ignore = ign_t; }
    __syncthreads();
    if (tid == 0) {
        LossRow r = swave[0];
        for (int k = 1; k < LOSS_T / 64; ++k) { r.giou += swave[k].giou; r.conf += swave[k].conf; r.cls += swave[k].cls; r.ignore += swave[k].ignore; }
        a.rows[blockIdx.x] = r;
    }
    if constexpr (GRAD) {
        // Phase 2: the workgroup's predictions are LOSS_T consecutive rows of dfeats (fewer in the last workgroup): one element per
        // lane and step, lane-consecutive addresses.  (r, c) = (row inside the workgroup, channel) of element e, stepped without a
        // division.  Class logits and class bits are read only where om != 0; every other element is stored without a load.
        const int nel = min(LOSS_T, a.total - (int)blockIdx.x * LOSS_T) * row;
        const size_t base = (size_t)blockIdx.x * LOSS_T * row;
        const float up = a.upstream ? *a.upstream : 1.0f;
        const float mf = (float)a.batch;
        const int dq = LOSS_T / row, dr = LOSS_T - dq * row;
        int r = tid / row, c = tid - r * row;
        for (int e = tid; e < nel; e += LOSS_T) {
            float v;
            if (c < 5) {
                v = sgrad[c][r];
            } else {
                const float om = sgrad[5][r];
                v = 0.0f;
                if (om != 0.0f) v = (om * (yr_sigmoid(a.feats[base + e]) - a.y_true[base + e])) / mf;   // :658-662
            }
            a.dfeats[base + e] = v * up;
            r += dq;
            c += dr;
            if (c >= row) { c -= row; ++r; }
        }
    }
}

// One workgroup.  Lane i adds rows i, i+256, ... in ascending order, then the same fixed tree as above; divide by B (:662-668),
// round once to float32.  `loss` is rounded from the float64 sum of the three terms, not from their float32 values.
__global__ __launch_bounds__(LOSS_T) void loss_final_kernel(LossArgs a) {
    __shared__ LossRow swave[LOSS_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double g = 0.0, c = 0.0, k = 0.0;
    long long ig = 0;
    for (int r = tid; r < a.nrows; r += LOSS_T) {
        const LossRow v = a.rows[r];
        g += v.giou; c += v.conf; k += v.cls; ig += v.ignore;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        g += __shfl_xor(g, o);
        c += __shfl_xor(c, o);
        k += __shfl_xor(k, o);
        ig += __shfl_xor(ig, o);
    }
    if (lane == 0) { swave[wave].giou = g; swave[wave].conf = c; swave[wave].cls = k; swave[wave].ignore = ig; }
    __syncthreads();
    if (tid == 0) {
        LossRow r = swave[0];
        for (int i = 1; i < LOSS_T / 64; ++i) { r.giou += swave[i].giou; r.conf += swave[i].conf; r.cls += swave[i].cls; r.ignore += swave[i].ignore; }
        const double mf = (double)a.batch;
        const double gl = r.giou / mf, cl = r.conf / mf, kl = r.cls / mf;
        a.out5[0] = (float)(gl + cl + kl);
        a.out5[1] = (float)gl;
        a.out5[2] = (float)cl;
        a.out5[3] = (float)kl;
        a.out5[4] = (float)r.ignore;
    }
}

static inline size_t loss_rows_offset(long long total) { return LOSS_HEADER + (size_t)total * sizeof(float4); }

extern "C" size_t yr_yolo_loss_workspace_bytes(int batch, int gh, int gw, int num_anchors) {
    if (batch <= 0 || gh <= 0 || gw <= 0 || num_anchors <= 0) return 0;
    const long long total = (long long)batch * gh * gw * num_anchors;
    return loss_rows_offset(total) + (size_t)((total + LOSS_T - 1) / LOSS_T) * sizeof(LossRow);
}

static int loss_launch(const float* feats, const float* y_true, int batch, int gh, int gw, int num_anchors, int num_classes,
                       const float* anchors_host, int in_h, int in_w, float ignore_thresh, void* workspace, size_t workspace_bytes,
                       const float* upstream, float* out5, float* dfeats, bool grad, void* stream) {
    YR_REQUIRE(feats && y_true && anchors_host && workspace && out5, "yolo_loss: null pointer");
    YR_REQUIRE(!grad || dfeats, "yolo_loss_grad: null pointer (dfeats)");
    YR_REQUIRE(num_anchors >= 1 && num_anchors <= 8, "yolo_loss: num_anchors must be 1..8");
    YR_REQUIRE(batch > 0 && gh > 0 && gw > 0 && num_classes >= 0 && in_h > 0 && in_w > 0, "yolo_loss: bad sizes");
    const long long total = (long long)batch * gh * gw * num_anchors;
    YR_REQUIRE(total * (num_classes + 5) < (1ll << 31), "yolo_loss: more than 2^31 logits");
    const size_t need = yr_yolo_loss_workspace_bytes(batch, gh, gw, num_anchors);
    YR_REQUIRE(workspace_bytes >= need, "yolo_loss: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    YR_REQUIRE(((uintptr_t)workspace) % 16 == 0, "yolo_loss: workspace not 16-byte aligned");
    LossArgs a;
    a.feats = feats; a.y_true = y_true;
    for (int k = 0; k < 8; ++k) {
        a.anchors[k][0] = k < num_anchors ? anchors_host[k * 2] : 0.0f;
        a.anchors[k][1] = k < num_anchors ? anchors_host[k * 2 + 1] : 0.0f;
    }
    a.gh = gh; a.gw = gw; a.A = num_anchors; a.C = num_classes; a.in_h = in_h; a.in_w = in_w; a.batch = batch;
    a.total = (int)total;
    a.ignore_thresh = ignore_thresh;
    char* ws = (char*)workspace;
    a.count = (unsigned*)ws;
    a.list = (float4*)(ws + LOSS_HEADER);
    a.rows = (LossRow*)(ws + loss_rows_offset(total));
    a.nrows = (int)((total + LOSS_T - 1) / LOSS_T);
    a.out5 = out5;
    a.dfeats = grad ? dfeats : nullptr;
    a.upstream = grad ? upstream : nullptr;
    hipStream_t s = (hipStream_t)stream;
    YR_CHECK_HIP(hipMemsetAsync(a.count, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(loss_compact_kernel, dim3(a.nrows), dim3(LOSS_T), 0, s, a);
    YR_LAUNCH_CHECK();
    if (grad)
        hipLaunchKernelGGL(loss_main_kernel<true>, dim3(a.nrows), dim3(LOSS_T), 0, s, a);
    else
        hipLaunchKernelGGL(loss_main_kernel<false>, dim3(a.nrows), dim3(LOSS_T), 0, s, a);
    YR_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(LOSS_T), 0, s, a);
    YR_LAUNCH_CHECK();
    return YR_OK;
}

extern "C" int yr_yolo_loss(const float* feats, const float* y_true, int batch, int gh, int gw, int num_anchors,
                            int num_classes, const float* anchors_host, int in_h, int in_w, float ignore_thresh,
                            void* workspace, size_t workspace_bytes, float* out5, void* stream) {
    return loss_launch(feats, y_true, batch, gh, gw, num_anchors, num_classes, anchors_host, in_h, in_w, ignore_thresh, workspace,
                       workspace_bytes, nullptr, out5, nullptr, false, stream);
}

extern "C" int yr_yolo_loss_grad(const float* feats, const float* y_true, int batch, int gh, int gw, int num_anchors,
                                 int num_classes, const float* anchors_host, int in_h, int in_w, float ignore_thresh,
                                 void* workspace, size_t workspace_bytes, const float* upstream_dev, float* out5, float* dfeats,
                                 void* stream) {
    return loss_launch(feats, y_true, batch, gh, gw, num_anchors, num_classes, anchors_host, in_h, in_w, ignore_thresh, workspace,
                       workspace_bytes, upstream_dev, out5, dfeats, true, stream);
}
