// tf.image.random_jpeg_quality on the device: code/yolo3/utils.py:228-230, the last image step of get_random_data(train=True), for
// a batch of float32 [B,H,W,3] canvases in place, one quality per image.  A JPEG encode followed by a decode without the
// bitstream (entropy coding is lossless): what is left is integer arithmetic, every piece as libjpeg's text has it and as
// tests/jpeg_ref.py restates it (that NumPy text, pinned byte for byte against Pillow on libjpeg-turbo, is the definition):
//   a  float -> uint8   convert_image_dtype(saturate=True): trunc(min(max(x * 255.5f, 0), 255))
//   b  RGB -> YCbCr     jccolor.c, 16-bit fixed point
//   c  chroma 2x2 mean  jcsample.c h2v2_downsample, bias 1, 2, 1, 2 along a row
//   d  tables           Annex K scaled by jpeg_quality_scaling, clamped to 1..255 (force_baseline)
//   e  forward DCT      jfdctint.c on sample - 128: rows (<< 2, descale 11), columns (descale 15, even outputs descale 2)
//   f  quantise         c = sign(v) * ((|v| + (d >> 1)) / d), d = 8 t
//   g  dequantise, inverse DCT   jidctint.c: columns (descale 11), rows (descale 18), + 128, clamp
//   h  chroma upsample  jdsample.c h2v2_fancy_upsample: 3/4 near + 1/4 far, vertically then horizontally
//   i  YCbCr -> RGB     jdcolor.c, clamp
//   j  uint8 -> float   u * (1 / 255)f
// H and W are multiples of 16 (the network input is a multiple of 32): whole 16x16 MCUs, none of libjpeg's edge rules.
//
// Two launches with a workspace between them - an output pixel needs the decoded chroma of up to eight neighbouring MCUs, whose
// source pixels a single in-place launch would already have overwritten:
//   jpeg_code_kernel    steps a-g.  One wave per MCU, four MCUs per workgroup, grid (ceil(MCUs / 4), B).  A lane loads four pixels
//                       of one MCU row (three 16-byte loads), converts, averages the chroma with its neighbour row (one xor shuffle)
//                       and stages sample - 128 of the six 8x8 blocks (4 Y, Cb, Cr) in LDS.  Then one lane per 8-point row: 48 of
//                       the 64 lanes run the row pass; transposed through LDS, one lane per column runs the forward column pass,
//                       quantises, dequantises and runs the inverse column pass without leaving its registers; transposed again,
//                       one lane per row runs the inverse row pass and stores its eight decoded bytes with one 8-byte store.
//                       The divisors of the image's quality are built once per workgroup in LDS with a 32-bit magic multiplier each.
//   jpeg_finish_kernel  steps h-j.  A lane owns four pixels of a row: one 4-byte Y load, per chroma plane and row one aligned 4-byte
//                       load plus the one byte beyond it, three 16-byte stores.  Indices clamped to the plane give libjpeg's edge
//                       rules: at the ends "far" is the sample itself.
// Workspace: decoded Y [B,H,W], Cb and Cr [B,H/2,W/2], uint8.  Every byte launch 2 reads is written by launch 1 of the same call.
// No atomics, no float arithmetic between a and j, no host synchronisation.
#include "yr_common.h"

#define JPEG_T 256
#define JPEG_WAVES (JPEG_T / 64)
#define JPEG_LD 9                      // ints per block row in LDS: 8 + 1, the row and the column pass both spread over the banks
#define JPEG_BLK (8 * JPEG_LD)

__constant__ unsigned char jpeg_base[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// FIX13(v) = int(v * 8192 + 0.5), jfdctint.c / jidctint.c
#define F_0_298631336 2446
#define F_0_390180644 3196
#define F_0_541196100 4433
#define F_0_765366865 6270
#define F_0_899976223 7373
#define F_1_175875602 9633
#define F_1_501321110 12299
#define F_1_847759065 15137
#define F_1_961570560 16069
#define F_2_053119869 16819
#define F_2_562915447 20995
#define F_3_072711026 25172

struct JpegArgs {
    float* img;                 // [B,H,W,3]
    const int32_t* quality;     // [B]
    unsigned char* y;           // [B,H,W]
    unsigned char* cb;          // [B,H/2,W/2]
    unsigned char* cr;
    int H, W;
    int mw;                     // MCUs per row
    unsigned mcus;              // MCUs per image
    unsigned nquad;             // H * W / 4
};

__device__ __forceinline__ int jpeg_descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int jpeg_clamp255(int v) { return min(max(v, 0), 255); }
__device__ __forceinline__ int jpeg_u8(float x) { return (int)fminf(fmaxf(x * 255.5f, 0.0f), 255.0f); }

// jpeg_fdct_islow, one 8-point pass in place; FIRST: pass 1 (rows), else pass 2 (columns)
template <bool FIRST>
__device__ __forceinline__ void jpeg_fdct8(int* d) {
    const int n = FIRST ? 11 : 15;
    int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (FIRST) { d[0] = (tmp10 + tmp11) * 4; d[4] = (tmp10 - tmp11) * 4; }
    else { d[0] = jpeg_descale(tmp10 + tmp11, 2); d[4] = jpeg_descale(tmp10 - tmp11, 2); }
    int z1 = (tmp12 + tmp13) * F_0_541196100;
    d[2] = jpeg_descale(z1 + tmp13 * F_0_765366865, n);
    d[6] = jpeg_descale(z1 - tmp12 * F_1_847759065, n);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * F_1_175875602;
    tmp4 *= F_0_298631336; tmp5 *= F_2_053119869; tmp6 *= F_3_072711026; tmp7 *= F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447;
    z3 = z3 * -F_1_961570560 + z5; z4 = z4 * -F_0_390180644 + z5;
    d[7] = jpeg_descale(tmp4 + z1 + z3, n);
    d[5] = jpeg_descale(tmp5 + z2 + z4, n);
    d[3] = jpeg_descale(tmp6 + z2 + z3, n);
    d[1] = jpeg_descale(tmp7 + z1 + z4, n);
}

// jpeg_idct_islow, one 8-point pass in place; FIRST: pass 1 (columns), else pass 2 (rows)
template <bool FIRST>
__device__ __forceinline__ void jpeg_idct8(int* d) {
    const int n = FIRST ? 11 : 18;
    int z2 = d[2], z3 = d[6];
    int z1 = (z2 + z3) * F_0_541196100;
    int tmp2 = z1 - z3 * F_1_847759065, tmp3 = z1 + z2 * F_0_765366865;
    int tmp0 = (d[0] + d[4]) * 8192, tmp1 = (d[0] - d[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7]; tmp1 = d[5]; tmp2 = d[3]; tmp3 = d[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F_1_175875602;
    tmp0 *= F_0_298631336; tmp1 *= F_2_053119869; tmp2 *= F_3_072711026; tmp3 *= F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447;
    z3 = z3 * -F_1_961570560 + z5; z4 = z4 * -F_0_390180644 + z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    d[0] = jpeg_descale(tmp10 + tmp3, n); d[7] = jpeg_descale(tmp10 - tmp3, n);
    d[1] = jpeg_descale(tmp11 + tmp2, n); d[6] = jpeg_descale(tmp11 - tmp2, n);
    d[2] = jpeg_descale(tmp12 + tmp1, n); d[5] = jpeg_descale(tmp12 - tmp1, n);
    d[3] = jpeg_descale(tmp13 + tmp0, n); d[4] = jpeg_descale(tmp13 - tmp0, n);
}

__global__ __launch_bounds__(JPEG_T) void jpeg_code_kernel(JpegArgs a) {
    __shared__ int blk[JPEG_WAVES][6 * JPEG_BLK];      // per wave: Y00, Y01, Y10, Y11, Cb, Cr, rows of JPEG_LD ints
    __shared__ int qt[2][64];                          // the divisors t of this image: luminance, chrominance
    __shared__ unsigned qm[2][64];                     // floor(2^32 / (8 t)) + 1 (2^32 / (8 t) for a power of two)
    const unsigned b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned m = blockIdx.x * (unsigned)JPEG_WAVES + wave;
    const bool live = m < a.mcus;                      // (uniform over the wave)
    int* mine = blk[wave];
    if (threadIdx.x < 128) {
        const int q = min(max(a.quality[b], 1), 100);
        const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
        const int t = min(max(((int)jpeg_base[threadIdx.x >> 6][lane] * scale + 50) / 100, 1), 255);
        qt[threadIdx.x >> 6][lane] = t;
        // n / d for n * d < 2^32 is the high word of n * M: M = 2^32 / d + e, 0 <= e <= 1, and n * e * d < 2^32
        qm[threadIdx.x >> 6][lane] = 0xFFFFFFFFu / (unsigned)(8 * t) + 1u;
    }
    const int my = live ? (int)(m / (unsigned)a.mw) : 0, mx = live ? (int)(m - (unsigned)my * (unsigned)a.mw) : 0;
    if (live) {
        // steps a-c: lane = row (lane >> 2) of the MCU, pixels 4 * (lane & 3) ...
        const int r = lane >> 2, c = (lane & 3) * 4;
        const size_t pix = ((size_t)b * a.H + (size_t)(my * 16 + r)) * a.W + (size_t)(mx * 16 + c);
        const float4* p4 = reinterpret_cast<const float4*>(a.img + pix * 3);
        const float4 i0 = p4[0], i1 = p4[1], i2 = p4[2];
        const float v[12] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w, i2.x, i2.y, i2.z, i2.w};
        int* yb = mine + ((r >> 3) * 2 + (c >> 3)) * JPEG_BLK + (r & 7) * JPEG_LD + (c & 7);
        int cbs[2], crs[2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int R = jpeg_u8(v[3 * j]), G = jpeg_u8(v[3 * j + 1]), B = jpeg_u8(v[3 * j + 2]);
            yb[j] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
            const int cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
            const int cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
            if (j & 1) { cbs[j >> 1] += cb; crs[j >> 1] += cr; }
            else { cbs[j >> 1] = cb; crs[j >> 1] = cr; }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {      // the neighbour row of the 2x2 block sits four lanes away
            cbs[k] += __shfl_xor(cbs[k], 4);
            crs[k] += __shfl_xor(crs[k], 4);
        }
        if ((r & 1) == 0) {
            int* cbb = mine + 4 * JPEG_BLK + (r >> 1) * JPEG_LD + (c >> 1);
            cbb[0] = ((cbs[0] + 1) >> 2) - 128; cbb[1] = ((cbs[1] + 2) >> 2) - 128;      // (c >> 1 is even: bias 1, then 2)
            cbb[JPEG_BLK] = ((crs[0] + 1) >> 2) - 128; cbb[JPEG_BLK + 1] = ((crs[1] + 2) >> 2) - 128;
        }
    }
    __syncthreads();
    const int block = lane >> 3, k8 = lane & 7;        // lanes 0..47: one 8-point row or column of block 0..5
    const bool work = live && lane < 48;
    int d[8];
    if (work) {      // step e, rows
        int* row = mine + block * JPEG_BLK + k8 * JPEG_LD;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = row[k];
        jpeg_fdct8<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) row[k] = d[k];
    }
    __syncthreads();
    if (work) {      // step e, columns; steps f and g up to the inverse column pass
        int* col = mine + block * JPEG_BLK + k8;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = col[k * JPEG_LD];
        jpeg_fdct8<false>(d);
        const int tab = block >= 4;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int t = qt[tab][k * 8 + k8];
            const unsigned n = (unsigned)abs(d[k]) + (unsigned)(4 * t);
            const int c = (int)__umulhi(n, qm[tab][k * 8 + k8]);
            d[k] = (d[k] < 0 ? -c : c) * t;
        }
        jpeg_idct8<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) col[k * JPEG_LD] = d[k];
    }
    __syncthreads();
    if (work) {      // step g, rows: eight decoded bytes of one block row
        const int* row = mine + block * JPEG_BLK + k8 * JPEG_LD;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = row[k];
        jpeg_idct8<false>(d);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (unsigned)jpeg_clamp255(d[k] + 128) << (8 * k);
            hi |= (unsigned)jpeg_clamp255(d[k + 4] + 128) << (8 * k);
        }
        unsigned char* o;
        if (block < 4) o = a.y + ((size_t)b * a.H + (size_t)(my * 16 + (block >> 1) * 8 + k8)) * a.W + (size_t)(mx * 16 + (block & 1) * 8);
        else o = (block == 4 ? a.cb : a.cr) + ((size_t)b * (a.H >> 1) + (size_t)(my * 8 + k8)) * (a.W >> 1) + (size_t)(mx * 8);
        *reinterpret_cast<uint2*>(o) = make_uint2(lo, hi);
    }
}

// the four chroma samples around output pixels 4 j .. 4 j + 3 of one plane row: s[i0 - 1], s[i0], s[i0 + 1], s[i0 + 2], i0 = 2 j,
// indices clamped to the row.  One aligned word holds three of them, the fourth is the byte before or after it.
__device__ __forceinline__ void jpeg_chroma4(const unsigned char* row, int j, int cw, int* s) {
    const int i0 = 2 * j;
    const unsigned w = *reinterpret_cast<const unsigned*>(row + (i0 & ~3));
    if (j & 1) {
        s[0] = (w >> 8) & 255; s[1] = (w >> 16) & 255; s[2] = w >> 24;
        s[3] = row[min(i0 + 2, cw - 1)];
    } else {
        s[0] = row[max(i0 - 1, 0)];
        s[1] = w & 255; s[2] = (w >> 8) & 255; s[3] = (w >> 16) & 255;
    }
}

__global__ __launch_bounds__(JPEG_T) void jpeg_finish_kernel(JpegArgs a) {
    const unsigned b = blockIdx.y;
    const unsigned q = blockIdx.x * (unsigned)JPEG_T + threadIdx.x;
    if (q >= a.nquad) return;
    const unsigned r = q * 4u;
    const int y = (int)(r / (unsigned)a.W), x = (int)(r - (unsigned)y * (unsigned)a.W);
    const int ch = a.H >> 1, cw = a.W >> 1;
    const int near = y >> 1, far = min(max((y & 1) ? near + 1 : near - 1, 0), ch - 1);
    const unsigned yw = *reinterpret_cast<const unsigned*>(a.y + ((size_t)b * a.H + (size_t)y) * a.W + (size_t)x);
    int c[2][4];      // step h for Cb, Cr: s = 3 near + far, then the same filter along the row
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const unsigned char* plane = (p ? a.cr : a.cb) + (size_t)b * ch * cw;
        int n4[4], f4[4], s[4];
        jpeg_chroma4(plane + (size_t)near * cw, x >> 2, cw, n4);
        jpeg_chroma4(plane + (size_t)far * cw, x >> 2, cw, f4);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = 3 * n4[k] + f4[k];
        c[p][0] = (3 * s[1] + s[0] + 8) >> 4;
        c[p][1] = (3 * s[1] + s[2] + 7) >> 4;
        c[p][2] = (3 * s[2] + s[1] + 8) >> 4;
        c[p][3] = (3 * s[2] + s[3] + 7) >> 4;
    }
    float v[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {      // steps i, j
        const int Y = (int)((yw >> (8 * j)) & 255u), cb = c[0][j] - 128, cr = c[1][j] - 128;
        const int R = jpeg_clamp255(Y + ((91881 * cr + 32768) >> 16));
        const int G = jpeg_clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
        const int B = jpeg_clamp255(Y + ((116130 * cb + 32768) >> 16));
        v[3 * j] = (float)R * (1.0f / 255.0f); v[3 * j + 1] = (float)G * (1.0f / 255.0f); v[3 * j + 2] = (float)B * (1.0f / 255.0f);
    }
    float4* o4 = reinterpret_cast<float4*>(a.img + ((size_t)b * a.nquad + q) * 12);
    o4[0] = make_float4(v[0], v[1], v[2], v[3]);
    o4[1] = make_float4(v[4], v[5], v[6], v[7]);
    o4[2] = make_float4(v[8], v[9], v[10], v[11]);
}

extern "C" size_t yr_jpeg_workspace_bytes(int batch, int H, int W) {
    if (batch <= 0 || H <= 0 || W <= 0) return 0;
    return ((size_t)batch * H * W * 3 / 2 + 15) & ~(size_t)15;
}

extern "C" int yr_jpeg_roundtrip_batch(float* images, const int32_t* quality, int batch, int H, int W, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    YR_REQUIRE(images && quality && workspace, "jpeg_roundtrip_batch: null pointer");
    YR_REQUIRE(batch > 0 && batch < 65536 && H > 0 && W > 0, "jpeg_roundtrip_batch: bad arguments (batch %d, images %dx%d)", batch, H, W);
    YR_REQUIRE(H % 16 == 0 && W % 16 == 0, "jpeg_roundtrip_batch: H and W must be multiples of 16 (whole MCUs), not %dx%d", H, W);
    YR_REQUIRE((long long)batch * H * W < (1ll << 31), "jpeg_roundtrip_batch: more than 2^31 pixels");
    YR_REQUIRE(((uintptr_t)images | (uintptr_t)workspace) % 16 == 0 && (uintptr_t)quality % 4 == 0,
               "jpeg_roundtrip_batch: images and workspace must be 16-byte aligned, quality 4-byte aligned");
    YR_REQUIRE(workspace_bytes >= yr_jpeg_workspace_bytes(batch, H, W), "jpeg_roundtrip_batch: the workspace needs %zu bytes (yr_jpeg_workspace_bytes), got %zu",
               yr_jpeg_workspace_bytes(batch, H, W), workspace_bytes);
    JpegArgs a;
    const size_t plane = (size_t)batch * H * W;
    a.img = images; a.quality = quality;
    a.y = (unsigned char*)workspace; a.cb = a.y + plane; a.cr = a.cb + plane / 4;
    a.H = H; a.W = W; a.mw = W / 16;
    a.mcus = (unsigned)((H / 16) * (W / 16));
    a.nquad = (unsigned)((long long)H * W / 4);
    hipLaunchKernelGGL(jpeg_code_kernel, dim3((a.mcus + JPEG_WAVES - 1) / JPEG_WAVES, (unsigned)batch), dim3(JPEG_T), 0, (hipStream_t)stream, a);
    YR_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_finish_kernel, dim3((a.nquad + JPEG_T - 1) / JPEG_T, (unsigned)batch), dim3(JPEG_T), 0, (hipStream_t)stream, a);
    YR_LAUNCH_CHECK();
    return YR_OK;
}
