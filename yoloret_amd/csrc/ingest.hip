// Ragged batched ingest: B decoded uint8 images of DIFFERENT sizes, packed back to back in one device buffer, -> the float32
// [B,H,W,3] network input in one launch, with per-image geometry in either of the reference's two letterbox rules, and - in the
// same launch - the ground-truth boxes of the validation pipeline mapped into the network input.  Replaces, after the host-side
// JPEG/PNG decode:
//   YR_INGEST_LETTERBOX  code/yolo.py:105-112 + code/yolo3/utils.py:67-83 (letterbox_image) per image: the geometry and the bytes
//                        of yr_letterbox (preprocess.hip);
//   YR_INGEST_VALIDATE   code/yolo3/utils.py:239-295, get_random_data(train=False, zoom_in=False), as called by
//                        Dataset.parse_text (code/yolo3/data.py:71-121): float32 geometry, the pad offset truncated from the
//                        UNTRUNCATED size, resize + pad (:246-252), the final clip_by_value(0, 1) (:277), and the boxes: mapped with
//                        the untruncated values (:253-256), clipped (:258-273), filtered by w > 1 and h > 1 (:289-291), cut to
//                        max_boxes (:292-293).
// The arithmetic of both geometries lives in ONE place, the host function yr_ingest_geometry; the kernel reads its table.
//
// One kernel, one launch, no workspace, no atomics, no float accumulation: the same call gives the same bytes.
//   * image workgroups: a lane owns four consecutive pixels of the flat [B*H*W] pixel order = 12 floats = three 16-byte stores
//     (48 q bytes from a 16-byte aligned base: aligned for every H and W; the existing kernel spends three scalar stores per pixel).
//     The pixel's (image, row, column) is divided out once per lane and stepped from there; the geometry of an image is fetched
//     when the lane enters it.  Per pixel the operations and their order are letterbox_kernel's (u8 * (1/255), bilinear with
//     half-pixel centres), so LETTERBOX mode repeats its bytes.  The last lane writes the up to three pixels behind the last
//     whole quad with scalar stores.
//   * box workgroups (VALIDATE mode with boxes only): one per image behind the image workgroups, lane = input row.  The order-
//     preserving compaction is a ballot per wave and a prefix over the four waves, as in labels.hip.
#include "yr_common.h"
#include "datapath_common.h"

#define ING_T YR_INGEST_MAX_BOXES   // lanes of a workgroup = input rows per image

struct IngArgs {
    const unsigned char* src;
    const yr_ingest_geom* geom;
    float* dst;
    int H, W, clip;
    unsigned npix;              // B * H * W < 2^31
    unsigned img_blocks;
    const float* boxes_in;      // [B,max_in,5]
    const int32_t* box_count;   // [B]
    int max_in;
    float* boxes_out;           // [B,max_boxes,5]
    int32_t* kept;              // [B] or null
    int max_boxes;
};

struct IngGeo {
    const unsigned char* src;
    int ih, iw, nh, nw, dy, dx;
    float sy, sx;               // ih/nh, iw/nw  (CalculateResizeScale)
};

__device__ __forceinline__ IngGeo ing_geo(const IngArgs& a, unsigned b) {
    const yr_ingest_geom* g = a.geom + b;
    IngGeo o;
    o.src = a.src + g->src_off;
    o.ih = g->ih; o.iw = g->iw; o.nh = g->nh; o.nw = g->nw; o.dy = g->dy; o.dx = g->dx;
    o.sy = (float)o.ih / (float)o.nh; o.sx = (float)o.iw / (float)o.nw;
    return o;
}

// one pixel of the network input: the window, the resize (datapath_common.h), then VALIDATE's clip (utils.py:277)
__device__ __forceinline__ void ing_pixel(const IngGeo& g, int y, int x, bool clip, float* o) {
    const int ry = y - g.dy, rx = x - g.dx;
    if (ry < 0 || ry >= g.nh || rx < 0 || rx >= g.nw) { o[0] = o[1] = o[2] = 0.0f; return; }
    yr_resize_pixel(g.src, g.ih, g.iw, g.sy, g.sx, ry, rx, o);
    if (clip) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = fmaxf(fminf(o[c], 1.0f), 0.0f);
    }
}

// the box workgroup of image b: datapath_common.h (shared with augment.hip), without the flip
__device__ __forceinline__ void ing_boxes(const IngArgs& a, unsigned b) {
    const yr_ingest_geom* g = a.geom + b;
    YrBoxMap m;
    m.boxes_in = a.boxes_in; m.box_count = a.box_count; m.max_in = a.max_in; m.boxes_out = a.boxes_out; m.kept = a.kept;
    m.max_boxes = a.max_boxes; m.H = a.H; m.W = a.W;
    yr_map_boxes(m, b, (float)g->ih, (float)g->iw, g->nh_f, g->nw_f, g->dy_f, g->dx_f, false);
}

__global__ __launch_bounds__(ING_T) void ingest_kernel(IngArgs a) {
    if (blockIdx.x >= a.img_blocks) { ing_boxes(a, blockIdx.x - a.img_blocks); return; }
    const unsigned q = blockIdx.x * (unsigned)ING_T + threadIdx.x;
    const unsigned nquad = (a.npix + 3u) >> 2;
    if (q >= nquad) return;
    const unsigned p = q * 4u, hw = (unsigned)(a.H * a.W);
    unsigned b = p / hw;
    const unsigned r = p - b * hw;
    int y = (int)(r / (unsigned)a.W), x = (int)(r - (unsigned)y * (unsigned)a.W);
    const unsigned left = a.npix - p;      // >= 1
    IngGeo g = ing_geo(a, b);
    float v[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if ((unsigned)j < left) ing_pixel(g, y, x, a.clip != 0, v + 3 * j);
        else v[3 * j] = v[3 * j + 1] = v[3 * j + 2] = 0.0f;
        if (++x == a.W) {
            x = 0;
            if (++y == a.H) {
                y = 0;
                if ((unsigned)(j + 1) < left) g = ing_geo(a, ++b);
            }
        }
    }
    float* o = a.dst + (size_t)p * 3;
    if (left >= 4u) {
        float4* o4 = reinterpret_cast<float4*>(o);
        o4[0] = make_float4(v[0], v[1], v[2], v[3]);
        o4[1] = make_float4(v[4], v[5], v[6], v[7]);
        o4[2] = make_float4(v[8], v[9], v[10], v[11]);
    } else {
#pragma unroll
        for (int e = 0; e < 9; ++e)
            if ((unsigned)e < left * 3u) o[e] = v[e];
    }
}

// The geometry of both rules for a ragged batch and where each image sits in the packed source: pure host arithmetic.
//   LETTERBOX  utils.py:76-79 - yr_letterbox_batch's host code: the ratio in float64, nh / nw truncated, offsets floor-divided;
//   VALIDATE   utils.py:152-155,239-242 in float32, TF's order: m = min(w / iw, h / ih); nh = ih * m; nw = iw * m;
//              dx = (w - nw) / 2; dy = (h - nh) / 2; :247-250 truncate those four (tf.cast to int32).
extern "C" int yr_ingest_geometry(int mode, int batch, const int32_t* dims_host, int H, int W, yr_ingest_geom* geom_host, int64_t* packed_bytes) {
    YR_REQUIRE(mode == YR_INGEST_LETTERBOX || mode == YR_INGEST_VALIDATE, "ingest_geometry: mode must be YR_INGEST_LETTERBOX or YR_INGEST_VALIDATE, not %d", mode);
    YR_REQUIRE(dims_host && geom_host, "ingest_geometry: null pointer");
    YR_REQUIRE(batch > 0 && batch < 65536, "ingest_geometry: batch must be 1..65535, not %d", batch);
    YR_REQUIRE(H > 0 && W > 0, "ingest_geometry: output %dx%d", H, W);
    int64_t off = 0;
    for (int b = 0; b < batch; ++b) {
        const int ih = dims_host[2 * b], iw = dims_host[2 * b + 1];
        YR_REQUIRE(ih > 0 && iw > 0, "ingest_geometry: image %d has size %dx%d", b, ih, iw);
        yr_ingest_geom g;
        g.src_off = off;
        g.ih = ih; g.iw = iw;
        g.reserved[0] = g.reserved[1] = g.reserved[2] = g.reserved[3] = 0;
        if (mode == YR_INGEST_LETTERBOX) {
            const double r = ((double)W / iw < (double)H / ih) ? (double)W / iw : (double)H / ih;
            g.nh = (int)((double)ih * r); g.nw = (int)((double)iw * r);
            g.dy = (H - g.nh) / 2; g.dx = (W - g.nw) / 2;
            g.nh_f = g.nw_f = g.dy_f = g.dx_f = 0.0f;
        } else {
            const float wf = (float)W, hf = (float)H, iwf = (float)iw, ihf = (float)ih;
            const float rw = wf / iwf, rh = hf / ihf;
            const float m = rw < rh ? rw : rh;
            g.nh_f = ihf * m; g.nw_f = iwf * m;
            g.dx_f = (wf - g.nw_f) / 2.0f; g.dy_f = (hf - g.nh_f) / 2.0f;
            g.nh = (int)g.nh_f; g.nw = (int)g.nw_f; g.dy = (int)g.dy_f; g.dx = (int)g.dx_f;
        }
        YR_REQUIRE(g.nh > 0 && g.nw > 0, "ingest_geometry: image %d (%dx%d) collapses to zero size at %dx%d", b, ih, iw, H, W);
        YR_REQUIRE(g.dy >= 0 && g.dx >= 0 && g.dy + g.nh <= H && g.dx + g.nw <= W, "ingest_geometry: image %d (%dx%d): the window leaves %dx%d", b, ih, iw, H, W);
        geom_host[b] = g;
        off = (off + (int64_t)ih * iw * 3 + 15) & ~(int64_t)15;
    }
    if (packed_bytes) *packed_bytes = off;
    return YR_OK;
}

extern "C" int yr_ingest_batch(int mode, const unsigned char* src_u8, const yr_ingest_geom* geom, int batch, float* dst, int H, int W,
                               const float* boxes_in, const int32_t* box_count, int max_in, float* boxes_out, int32_t* kept, int max_boxes,
                               void* stream) {
    YR_REQUIRE(mode == YR_INGEST_LETTERBOX || mode == YR_INGEST_VALIDATE, "ingest_batch: mode must be YR_INGEST_LETTERBOX or YR_INGEST_VALIDATE, not %d", mode);
    YR_REQUIRE(src_u8 && geom && dst, "ingest_batch: null pointer");
    YR_REQUIRE(batch > 0 && batch < 65536 && H > 0 && W > 0, "ingest_batch: bad arguments (batch %d, output %dx%d)", batch, H, W);
    YR_REQUIRE((long long)batch * H * W < (1ll << 31), "ingest_batch: more than 2^31 output pixels");
    YR_REQUIRE(((uintptr_t)src_u8 | (uintptr_t)geom | (uintptr_t)dst) % 16 == 0, "ingest_batch: source, table and output must be 16-byte aligned");
    IngArgs a;
    a.src = src_u8; a.geom = geom; a.dst = dst; a.H = H; a.W = W; a.clip = mode == YR_INGEST_VALIDATE;
    a.npix = (unsigned)((long long)batch * H * W);
    a.img_blocks = ((a.npix + 3u) / 4u + ING_T - 1) / ING_T;
    a.boxes_in = boxes_in; a.box_count = box_count; a.max_in = max_in; a.boxes_out = boxes_out; a.kept = kept; a.max_boxes = max_boxes;
    unsigned blocks = a.img_blocks;
    if (boxes_in != nullptr) {
        YR_REQUIRE(mode == YR_INGEST_VALIDATE, "ingest_batch: boxes are mapped in YR_INGEST_VALIDATE mode only");
        YR_REQUIRE(box_count && boxes_out, "ingest_batch: boxes without box_count or boxes_out");
        YR_REQUIRE(max_in >= 1 && max_in <= YR_INGEST_MAX_BOXES, "ingest_batch: max_in must be 1..%d, not %d", YR_INGEST_MAX_BOXES, max_in);
        YR_REQUIRE(max_boxes >= 1 && max_boxes <= (1 << 20), "ingest_batch: max_boxes must be 1..2^20, not %d", max_boxes);
        blocks += (unsigned)batch;
    }
    hipLaunchKernelGGL(ingest_kernel, dim3(blocks), dim3(ING_T), 0, (hipStream_t)stream, a);
    YR_LAUNCH_CHECK();
    return YR_OK;
}
