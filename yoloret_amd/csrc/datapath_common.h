// What the two data paths share (ingest.hip: letterbox_image and get_random_data(train=False); augment.hip: train=True).
//
// yr_resize_pixel: one pixel of tf.image.resize (bilinear, half-pixel centres, no antialias) of a decoded uint8 image, in
// letterbox_kernel's operation order (preprocess.hip): u8 * (1/255), then the two horizontal and the one vertical interpolation.
//
// yr_map_boxes: the box workgroup - one workgroup per image, lane = input row.  code/yolo3/utils.py:208-217 | :253-256 map a row
// with the UNTRUNCATED float32 geometry, left to right; under `flip` (train only, :212-217) (xmin, xmax) -> (w - xmax, w - xmin);
// then :258-273 clip (clip_by_value: the minimum first), :289-291 keep rows with w > 1 and h > 1 (both strict), :292-293 cut to
// max_boxes.  The order-preserving compaction is a ballot per wave and a prefix over the four waves, as in labels.hip.
#pragma once
#include "yr_common.h"

#define YR_BOX_T YR_INGEST_MAX_BOXES   // lanes of the workgroup = input rows per image

// (ry, rx): the pixel of the resized image; sy = ih / nh, sx = iw / nw (CalculateResizeScale)
__device__ __forceinline__ void yr_resize_pixel(const unsigned char* src, int ih, int iw, float sy, float sx, int ry, int rx, float* o) {
    const float inv255 = 1.0f / 255.0f;
    const float fy = ((float)ry + 0.5f) * sy - 0.5f, fx = ((float)rx + 0.5f) * sx - 0.5f;
    const float fly = floorf(fy), flx = floorf(fx);
    const int y0 = max((int)fly, 0), y1 = min((int)ceilf(fy), ih - 1);
    const int x0 = max((int)flx, 0), x1 = min((int)ceilf(fx), iw - 1);
    const float ly = fy - fly, lx = fx - flx;
    const unsigned char* p00 = src + ((size_t)y0 * iw + x0) * 3;
    const unsigned char* p01 = src + ((size_t)y0 * iw + x1) * 3;
    const unsigned char* p10 = src + ((size_t)y1 * iw + x0) * 3;
    const unsigned char* p11 = src + ((size_t)y1 * iw + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float tl = (float)p00[c] * inv255, tr = (float)p01[c] * inv255;
        const float bl = (float)p10[c] * inv255, br = (float)p11[c] * inv255;
        const float top = tl + (tr - tl) * lx;
        const float bot = bl + (br - bl) * lx;
        o[c] = top + (bot - top) * ly;
    }
}

struct YrBoxMap {
    const float* boxes_in;      // [B,max_in,5]
    const int32_t* box_count;   // [B]
    int max_in;
    float* boxes_out;           // [B,max_boxes,5]
    int32_t* kept;              // [B] or null
    int max_boxes;
    int H, W;
};

__device__ __forceinline__ void yr_map_boxes(const YrBoxMap& a, unsigned b, float ihf, float iwf, float nhf, float nwf, float dyf, float dxf, bool flip) {
    __shared__ int wkept[YR_BOX_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = a.box_count[b];
    n = n < 0 ? 0 : (n > a.max_in ? a.max_in : n);
    float x0 = 0.0f, y0 = 0.0f, x1 = 0.0f, y1 = 0.0f, label = 0.0f;
    bool keep = false;
    if (tid < n) {
        const float* t = a.boxes_in + ((size_t)b * a.max_in + tid) * 5;
        const float xmax = (float)(a.W - 1), ymax = (float)(a.H - 1);
        float mx0 = t[0] * nwf / iwf + dxf, mx1 = t[2] * nwf / iwf + dxf;
        if (flip) {
            const float wf = (float)a.W, f0 = wf - mx1, f1 = wf - mx0;      // w, not w - 1
            mx0 = f0; mx1 = f1;
        }
        x0 = fmaxf(fminf(mx0, xmax), 0.0f);
        y0 = fmaxf(fminf(t[1] * nhf / ihf + dyf, ymax), 0.0f);
        x1 = fmaxf(fminf(mx1, xmax), 0.0f);
        y1 = fmaxf(fminf(t[3] * nhf / ihf + dyf, ymax), 0.0f);
        label = t[4];
        keep = x1 - x0 > 1.0f && y1 - y0 > 1.0f;
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wkept[wave] = __popcll(m);
    __syncthreads();
    int rank = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int k = 0; k < YR_BOX_T / 64; ++k) {
        if (k < wave) rank += wkept[k];
        total += wkept[k];
    }
    const int nk = total < a.max_boxes ? total : a.max_boxes;
    float* out = a.boxes_out + (size_t)b * a.max_boxes * 5;
    if (keep && rank < nk) {
        float* e = out + (size_t)rank * 5;
        e[0] = x0; e[1] = y0; e[2] = x1; e[3] = y1; e[4] = label;
    }
    for (int e = nk * 5 + tid; e < a.max_boxes * 5; e += YR_BOX_T) out[e] = 0.0f;
    if (tid == 0 && a.kept != nullptr) a.kept[b] = nk;
}
