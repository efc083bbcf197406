// The training data transform on the device: code/yolo3/utils.py:170-237, get_random_data(train=True), for a ragged batch of
// decoded uint8 images packed back to back -> the float32 [B,H,W,3] network input and the mapped ground-truth boxes.
//   geometry  :171-181  ten uniform draws per image (j1, j2, scale, dx, dy, flip, hue, sat, gamma, contrast) -> yr_augment_geom.
//                       The arithmetic lives in ONE place, the host function yr_augment_geometry; the kernels read its table.
//   image     :182-206  resize to (int(nh), int(nw)) - the arithmetic ingest.hip runs -, crop, pad: never materialised, an
//                       output pixel maps back through flip, pad offset, crop offset and resize;
//             :212-217  flip of the whole padded canvas;
//             :218-227  random_hue, random_saturation, adjust_gamma, random_contrast with the table's scalars;  :277 the clip.
//   boxes     :208-217, then :258-293 - datapath_common.h, the workgroup ingest.hip runs, with the flip.
// random_jpeg_quality (:228-230) is a stage of its own behind these launches: jpeg.hip.  Not built: val, noise, blur, zoom_in.
//
// TensorFlow's adjust_hue / adjust_saturation kernels are restated here as tests/augment_ref.py restates them (that NumPy text is
// the definition under test): every operation one float32 operation in the same order, the build keeps -ffp-contract=off.
//
// Two launches, grid (blocks, B): a workgroup never straddles two images; a lane owns four pixels = three 16-byte stores.
//   aug_pixels_kernel   every pixel through gamma, stored; the three channel sums of the workgroup in a fixed tree (lane: pixel
//                       order; wave: xor butterfly; the four waves in order) -> its own slot [b][block][3] of the workspace.
//                       With the contrast stage off it clips and the workspace is not touched.
//   aug_finish_kernel   each workgroup adds its image's slots (lane t: slots t, t + 256, ... in order, then the same tree), divides
//                       by H * W, applies contrast and the clip in place; one extra workgroup per image maps the boxes.  With the
//                       contrast stage off it carries only the boxes (and is not launched without boxes).
// No atomics, no float accumulation whose order depends on scheduling: the same call gives the same bytes.
#include "yr_common.h"
#include "datapath_common.h"

#define AUG_T 256
static_assert(AUG_T == YR_BOX_T, "the box workgroup rides in aug_finish_kernel's grid");

struct AugArgs {
    const unsigned char* src;
    const yr_augment_geom* geom;
    float* dst;
    float* ws;                  // [B][blocks][3]
    int H, W, stages;
    unsigned nquad;             // H * W / 4
    unsigned blocks;            // image workgroups per image
    YrBoxMap box;
};

// adjust_hue: (r, g, b) -> (h in [0, 6), v_min, v_max), h += delta * 6, back
__device__ __forceinline__ void aug_hue(float* p, float delta6) {
    const float r = p[0], g = p[1], b = p[2];
    int cat;
    float vmax, vmid, vmin;
    if (r < g) {
        if (b < r) { cat = 1; vmax = g; vmid = r; vmin = b; }
        else if (b > g) { cat = 3; vmax = b; vmid = g; vmin = r; }
        else { cat = 2; vmax = g; vmid = b; vmin = r; }
    } else {
        if (b < g) { cat = 0; vmax = r; vmid = g; vmin = b; }
        else if (b > r) { cat = 4; vmax = b; vmid = r; vmin = g; }
        else { cat = 5; vmax = r; vmid = b; vmin = g; }
    }
    const float range = vmax - vmin;
    float h = 0.0f;
    if (vmax != vmin) {
        const float ratio = (vmid - vmin) / range;
        h = (float)cat + ((cat & 1) ? 1.0f - ratio : ratio);
    }
    h = h + delta6;
    while (h < 0.0f) h = h + 6.0f;
    while (h >= 6.0f) h = h - 6.0f;
    cat = (int)h;
    float ratio = h - (float)cat;
    if (cat & 1) ratio = 1.0f - ratio;
    vmid = vmin + ratio * range;
    switch (cat) {
        case 0: p[0] = vmax; p[1] = vmid; p[2] = vmin; break;
        case 1: p[0] = vmid; p[1] = vmax; p[2] = vmin; break;
        case 2: p[0] = vmin; p[1] = vmax; p[2] = vmid; break;
        case 3: p[0] = vmin; p[1] = vmid; p[2] = vmax; break;
        case 4: p[0] = vmid; p[1] = vmin; p[2] = vmax; break;
        default: p[0] = vmax; p[1] = vmin; p[2] = vmid; break;
    }
}

// adjust_saturation: RGB -> HSV, s = clamp(s * factor, 0, 1), HSV -> RGB
__device__ __forceinline__ void aug_saturation(float* p, float factor) {
    const float r = p[0], g = p[1], b = p[2];
    const float v = fmaxf(fmaxf(r, g), b);
    const float range = v - fminf(fminf(r, g), b);
    float s = v > 0.0f ? range / v : 0.0f;
    const float norm = 1.0f / (6.0f * range);
    float h;
    if (r == v) h = norm * (g - b);
    else if (g == v) h = norm * (b - r) + 2.0f / 6.0f;      // 2/6 and 4/6 are float32 quotients
    else h = norm * (r - g) + 4.0f / 6.0f;
    if (range <= 0.0f) h = 0.0f;
    if (h < 0.0f) h = h + 1.0f;
    s = fminf(1.0f, fmaxf(0.0f, s * factor));
    const float c = s * v, m = v - c, dh = h * 6.0f;
    float f = dh;
    while (f < 0.0f) f = f + 2.0f;
    while (f >= 2.0f) f = f - 2.0f;
    const float x = c * (1.0f - fabsf(f - 1.0f));
    float rr = 0.0f, gg = 0.0f, bb = 0.0f;
    switch ((int)dh) {
        case 0: rr = c; gg = x; break;
        case 1: rr = x; gg = c; break;
        case 2: gg = c; bb = x; break;
        case 3: gg = x; bb = c; break;
        case 4: rr = x; bb = c; break;
        case 5: rr = c; bb = x; break;
        default: break;
    }
    p[0] = rr + m; p[1] = gg + m; p[2] = bb + m;
}

// one pixel of the padded, flipped canvas through gamma: the resize ingest.hip runs (datapath_common.h) behind the window mapping
__device__ __forceinline__ void aug_pixel(const unsigned char* src, const yr_augment_geom& g, float sy, float sx, int W, int stages, int y, int x, float* o) {
    const int ux = g.flip ? W - 1 - x : x;      // the column of the canvas before the flip
    const int wy = y - g.py, wx = ux - g.px;
    if (wy < 0 || wy >= g.wh || wx < 0 || wx >= g.ww) { o[0] = o[1] = o[2] = 0.0f; }
    else {
        const int ry = wy + g.cy, rx = wx + g.cx;
        yr_resize_pixel(src, g.ih, g.iw, sy, sx, ry, rx, o);
    }
    // the colour steps see the padding too (zeros: grey at 0 through hue and saturation, 0 ** gamma = 0)
    if (stages & YR_AUG_HUE) aug_hue(o, g.hue6);
    if (stages & YR_AUG_SAT) aug_saturation(o, g.sat);
    if (stages & YR_AUG_GAMMA) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = powf(o[c], g.gamma);
    }
}

// three sums over the workgroup in a fixed tree; every thread receives the totals
__device__ __forceinline__ void aug_block_sum(float* s) {
    __shared__ float part[AUG_T / 64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = s[c] + __shfl_xor(s[c], d);
    }
    if (lane == 0) { part[wave][0] = s[0]; part[wave][1] = s[1]; part[wave][2] = s[2]; }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
}

__global__ __launch_bounds__(AUG_T) void aug_pixels_kernel(AugArgs a) {
    const unsigned b = blockIdx.y;
    const unsigned q = blockIdx.x * (unsigned)AUG_T + threadIdx.x;
    const bool contrast = (a.stages & YR_AUG_CONTRAST) != 0;
    float s[3] = {0.0f, 0.0f, 0.0f};
    if (q < a.nquad) {
        const yr_augment_geom g = a.geom[b];
        const unsigned char* src = a.src + g.src_off;
        const float sy = (float)g.ih / (float)g.rh, sx = (float)g.iw / (float)g.rw;
        const unsigned r = q * 4u;
        int y = (int)(r / (unsigned)a.W), x = (int)(r - (unsigned)y * (unsigned)a.W);
        float v[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            aug_pixel(src, g, sy, sx, a.W, a.stages, y, x, v + 3 * j);
            if (++x == a.W) { x = 0; ++y; }
        }
        if (contrast) {
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] = (v[c] + v[3 + c]) + (v[6 + c] + v[9 + c]);
        } else {
#pragma unroll
            for (int e = 0; e < 12; ++e) v[e] = fmaxf(fminf(v[e], 1.0f), 0.0f);
        }
        float4* o4 = reinterpret_cast<float4*>(a.dst + ((size_t)b * a.nquad + q) * 12);
        o4[0] = make_float4(v[0], v[1], v[2], v[3]);
        o4[1] = make_float4(v[4], v[5], v[6], v[7]);
        o4[2] = make_float4(v[8], v[9], v[10], v[11]);
    }
    if (!contrast) return;      // (uniform over the grid)
    aug_block_sum(s);
    const float mine = threadIdx.x == 0 ? s[0] : (threadIdx.x == 1 ? s[1] : s[2]);
    if (threadIdx.x < 3) a.ws[((size_t)b * a.blocks + blockIdx.x) * 3 + threadIdx.x] = mine;
}

__global__ __launch_bounds__(AUG_T) void aug_finish_kernel(AugArgs a) {
    const unsigned b = blockIdx.y;
    const bool contrast = (a.stages & YR_AUG_CONTRAST) != 0;
    if (!contrast || blockIdx.x >= a.blocks) {      // the box workgroup of image b (the only workgroup with the contrast stage off)
        const yr_augment_geom* g = a.geom + b;
        yr_map_boxes(a.box, b, (float)g->ih, (float)g->iw, g->nh_f, g->nw_f, g->dy_f, g->dx_f, g->flip != 0);
        return;
    }
    float s[3] = {0.0f, 0.0f, 0.0f};
    const float* slots = a.ws + (size_t)b * a.blocks * 3;
    for (unsigned k = threadIdx.x; k < a.blocks; k += AUG_T) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = s[c] + slots[(size_t)k * 3 + c];
    }
    aug_block_sum(s);
    const unsigned q = blockIdx.x * (unsigned)AUG_T + threadIdx.x;
    if (q >= a.nquad) return;
    const float n = (float)(a.nquad * 4u), f = a.geom[b].cont;
    const float mean[3] = {s[0] / n, s[1] / n, s[2] / n};
    float4* o4 = reinterpret_cast<float4*>(a.dst + ((size_t)b * a.nquad + q) * 12);
    const float4 i0 = o4[0], i1 = o4[1], i2 = o4[2];
    float v[12] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w, i2.x, i2.y, i2.z, i2.w};
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const float m = mean[e % 3];
        v[e] = fmaxf(fminf((v[e] - m) * f + m, 1.0f), 0.0f);
    }
    o4[0] = make_float4(v[0], v[1], v[2], v[3]);
    o4[1] = make_float4(v[4], v[5], v[6], v[7]);
    o4[2] = make_float4(v[8], v[9], v[10], v[11]);
}

static inline float aug_uniform(float u, float lo, float hi) { return lo + u * (hi - lo); }      // tf.random.uniform([], lo, hi)

// utils.py:171-181 and the draws of :212-227 in float32, TF's order; :183-198 truncate (tf.cast to int32).  A Python literal such
// as 1 - jitter reaches TensorFlow as a double and is rounded to float32 once: the bounds are computed in double here too.
extern "C" int yr_augment_geometry(int batch, const int32_t* dims_host, int H, int W, const float* draws_host, int stages,
                                   double jitter, double min_scale, double max_scale, double hue, double sat, double min_gamma, double max_gamma,
                                   double cont, yr_augment_geom* geom_host, int64_t* packed_bytes) {
    YR_REQUIRE(dims_host && draws_host && geom_host, "augment_geometry: null pointer");
    YR_REQUIRE(batch > 0 && batch < 65536, "augment_geometry: batch must be 1..65535, not %d", batch);
    YR_REQUIRE(H > 0 && W > 0, "augment_geometry: output %dx%d", H, W);
    YR_REQUIRE((stages & ~YR_AUG_ALL) == 0, "augment_geometry: unknown stage bits 0x%x", stages);
    YR_REQUIRE(jitter >= 0.0 && jitter < 1.0 && min_scale > 0.0 && max_scale >= min_scale, "augment_geometry: jitter %g must lie in [0, 1), 0 < min_scale %g <= max_scale %g", jitter, min_scale, max_scale);
    YR_REQUIRE(!(stages & YR_AUG_HUE) || (hue >= 0.0 && hue <= 0.5), "augment_geometry: hue %g must lie in [0, 0.5]", hue);
    YR_REQUIRE(!(stages & YR_AUG_SAT) || (sat >= 0.0 && sat <= 1.0), "augment_geometry: sat %g must lie in [0, 1]", sat);
    YR_REQUIRE(!(stages & YR_AUG_GAMMA) || (min_gamma >= 0.0 && max_gamma >= min_gamma), "augment_geometry: 0 <= min_gamma %g <= max_gamma %g", min_gamma, max_gamma);
    YR_REQUIRE(!(stages & YR_AUG_CONTRAST) || (cont >= 0.0 && cont <= 1.0), "augment_geometry: cont %g must lie in [0, 1]", cont);
    const float w = (float)W, h = (float)H;
    const float jlo = (float)(1.0 - jitter), jhi = (float)(1.0 + jitter);
    int64_t off = 0;
    for (int b = 0; b < batch; ++b) {
        const int ih = dims_host[2 * b], iw = dims_host[2 * b + 1];
        const float* u = draws_host + (size_t)b * 10;
        YR_REQUIRE(ih > 0 && iw > 0, "augment_geometry: image %d has size %dx%d", b, ih, iw);
        for (int k = 0; k < 10; ++k) YR_REQUIRE(u[k] - u[k] == 0.0f, "augment_geometry: image %d: draw %d is not finite", b, k);
        yr_augment_geom g;
        g.src_off = off;
        g.ih = ih; g.iw = iw;
        const float new_ar = (w / h) * (aug_uniform(u[0], jlo, jhi) / aug_uniform(u[1], jlo, jhi));
        const float scale = aug_uniform(u[2], (float)min_scale, (float)max_scale);
        float ratio = new_ar < 1.0f ? scale * new_ar : scale / new_ar;
        ratio = ratio > 1.0f ? ratio : 1.0f;
        g.clamped = ratio == 1.0f;
        const float nw = new_ar < 1.0f ? ratio * h : scale * w, nh = new_ar < 1.0f ? scale * h : ratio * w;
        const float dx = aug_uniform(u[3], 0.0f, w - nw), dy = aug_uniform(u[4], 0.0f, h - nh);
        g.nh_f = nh; g.nw_f = nw; g.dy_f = dy; g.dx_f = dx;
        const float big = 1073741824.0f;      // 2^30: everything below is truncated to int32
        YR_REQUIRE(nh < big && nw < big && dx > -big && dx < big && dy > -big && dy < big, "augment_geometry: image %d: resized size %g x %g at (%g, %g) is out of range", b, (double)nh, (double)nw, (double)dy, (double)dx);
        g.rh = (int)nh; g.rw = (int)nw;
        YR_REQUIRE(g.rh > 0 && g.rw > 0, "augment_geometry: image %d: the resized image %g x %g truncates to zero size", b, (double)nh, (double)nw);
        const float ndy = -dy > 0.0f ? -dy : 0.0f, ndx = -dx > 0.0f ? -dx : 0.0f;      // tf.math.maximum(-dy, 0)
        const float pdy = dy > 0.0f ? dy : 0.0f, pdx = dx > 0.0f ? dx : 0.0f;
        g.py = (int)pdy; g.px = (int)pdx;
        if (nw > w || nh > h) {      // crop_and_pad (:188-199)
            g.cy = (int)ndy; g.cx = (int)ndx;
            g.wh = H < g.rh ? H : g.rh; g.ww = W < g.rw ? W : g.rw;
            YR_REQUIRE(g.cy + g.wh <= g.rh && g.cx + g.ww <= g.rw, "augment_geometry: image %d: crop_to_bounding_box would fail: %dx%d at (%d, %d) of %dx%d", b, g.wh, g.ww, g.cy, g.cx, g.rh, g.rw);
        } else {
            g.cy = g.cx = 0; g.wh = g.rh; g.ww = g.rw;
        }
        YR_REQUIRE(g.py + g.wh <= H && g.px + g.ww <= W, "augment_geometry: image %d: pad_to_bounding_box would fail: %dx%d at (%d, %d) of %dx%d", b, g.wh, g.ww, g.py, g.px, H, W);
        g.flip = !(stages & YR_AUG_NOFLIP) && u[5] < 0.5f;
        g.hue6 = (stages & YR_AUG_HUE) ? aug_uniform(u[6], (float)-hue, (float)hue) * 6.0f : 0.0f;
        g.sat = (stages & YR_AUG_SAT) ? aug_uniform(u[7], (float)(1.0 - sat), (float)(1.0 + sat)) : 1.0f;
        g.gamma = (stages & YR_AUG_GAMMA) ? aug_uniform(u[8], (float)min_gamma, (float)max_gamma) : 1.0f;
        g.cont = (stages & YR_AUG_CONTRAST) ? aug_uniform(u[9], (float)(1.0 - cont), (float)(1.0 + cont)) : 1.0f;
        g.reserved[0] = g.reserved[1] = 0;
        geom_host[b] = g;
        off = (off + (int64_t)ih * iw * 3 + 15) & ~(int64_t)15;
    }
    if (packed_bytes) *packed_bytes = off;
    return YR_OK;
}

static unsigned aug_blocks(int H, int W) { return (unsigned)(((long long)H * W / 4 + AUG_T - 1) / AUG_T); }

extern "C" size_t yr_augment_workspace_bytes(int batch, int H, int W) {
    if (batch <= 0 || H <= 0 || W <= 0) return 0;
    return (((size_t)batch * aug_blocks(H, W) * 3 * sizeof(float)) + 15) & ~(size_t)15;
}

extern "C" int yr_augment_batch(const unsigned char* src_u8, const yr_augment_geom* geom, int batch, int stages, float* dst, int H, int W,
                                const float* boxes_in, const int32_t* box_count, int max_in, float* boxes_out, int32_t* kept, int max_boxes,
                                void* workspace, size_t workspace_bytes, void* stream) {
    YR_REQUIRE(src_u8 && geom && dst, "augment_batch: null pointer");
    YR_REQUIRE(batch > 0 && batch < 65536 && H > 0 && W > 0, "augment_batch: bad arguments (batch %d, output %dx%d)", batch, H, W);
    YR_REQUIRE((stages & ~YR_AUG_ALL) == 0, "augment_batch: unknown stage bits 0x%x", stages);
    YR_REQUIRE((long long)H * W % 4 == 0, "augment_batch: H * W must be a multiple of 4 (a lane owns four pixels of one image), not %dx%d", H, W);
    YR_REQUIRE((long long)batch * H * W < (1ll << 31), "augment_batch: more than 2^31 output pixels");
    YR_REQUIRE(((uintptr_t)src_u8 | (uintptr_t)geom | (uintptr_t)dst | (uintptr_t)workspace) % 16 == 0, "augment_batch: source, table, output and workspace must be 16-byte aligned");
    const bool contrast = (stages & YR_AUG_CONTRAST) != 0;
    YR_REQUIRE(!contrast || (workspace && workspace_bytes >= yr_augment_workspace_bytes(batch, H, W)),
               "augment_batch: the contrast stage needs a workspace of %zu bytes (yr_augment_workspace_bytes), got %zu", yr_augment_workspace_bytes(batch, H, W), workspace_bytes);
    AugArgs a;
    a.src = src_u8; a.geom = geom; a.dst = dst; a.ws = (float*)workspace; a.H = H; a.W = W; a.stages = stages;
    a.nquad = (unsigned)((long long)H * W / 4);
    a.blocks = aug_blocks(H, W);
    a.box.boxes_in = boxes_in; a.box.box_count = box_count; a.box.max_in = max_in; a.box.boxes_out = boxes_out; a.box.kept = kept;
    a.box.max_boxes = max_boxes; a.box.H = H; a.box.W = W;
    if (boxes_in != nullptr) {
        YR_REQUIRE(box_count && boxes_out, "augment_batch: boxes without box_count or boxes_out");
        YR_REQUIRE(max_in >= 1 && max_in <= YR_INGEST_MAX_BOXES, "augment_batch: max_in must be 1..%d, not %d", YR_INGEST_MAX_BOXES, max_in);
        YR_REQUIRE(max_boxes >= 1 && max_boxes <= (1 << 20), "augment_batch: max_boxes must be 1..2^20, not %d", max_boxes);
    }
    hipLaunchKernelGGL(aug_pixels_kernel, dim3(a.blocks, (unsigned)batch), dim3(AUG_T), 0, (hipStream_t)stream, a);
    YR_LAUNCH_CHECK();
    const unsigned fin = (contrast ? a.blocks : 0u) + (boxes_in != nullptr ? 1u : 0u);
    if (fin > 0) {
        hipLaunchKernelGGL(aug_finish_kernel, dim3(fin, (unsigned)batch), dim3(AUG_T), 0, (hipStream_t)stream, a);
        YR_LAUNCH_CHECK();
    }
    return YR_OK;
}
