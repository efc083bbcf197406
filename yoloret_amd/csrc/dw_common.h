// What the inference depthwise family shares, each rule stated once - depthwise.hip (dw_kernel: straight from global memory, every
// element type and stride; the dispatcher), depthwise_lds.hip (dwp_kernel: 16-bit, stride 1, a walk over LDS tiles) and
// depthwise_walk.hip (dwq_kernel: 16-bit 5 x 5, a walk down column blocks).  The three forms are bit-identical: float32
// accumulation in (ky, kx) order, BatchNorm, activation, one rounding on store.
//   host:   DwMap (the map as launch_depthwise_t hands it to the two 16-bit forms), dw_args_of (its copy into a kernel's argument
//           struct), DW_BY_16 (their element types), DW_BY_ACT (their three activation variants, each instantiation stated once);
//   device: of the two walking kernels - dw_f2 / dw_widen, dw_act, the dead offsets, one tap over a strip's four columns dw_tap4,
//           the row read-ahead dw_row_read / dw_row_next, the finish of an output row dw_finish_row.
#pragma once
#include "yr_common.h"
#include <cstdlib>

// ---------------------------------------------------------------- host side
// A stride-1 'SAME' depthwise op on a 16-bit map, by its numbers alone.
struct DwMap {
    int dtype;           // YR_BF16 | YR_F16
    const void* in;      // [B][H][W][ld_in] 16-bit
    const float *w, *scale, *shift;   // [K*K][ld_w] taps, BatchNorm
    void* out;           // [B][H][W][ld_out]
    int B, H, W, C8;     // C8 = ceil(C / 8): 16-byte channel vectors per pixel
    int ld_in, ld_w, ld_out;
    int pad_t, pad_l, act;
    float* part;         // squeeze-excite form: float32 channel sums of what each tile / (block, quantum) stored, or null
    int ld_part;
};
int yr_launch_depthwise_lds(const DwMap& m, int k, int part_rows, hipStream_t s);    // depthwise_lds.hip
int yr_launch_depthwise_walk(const DwMap& m, int k, int part_rows, hipStream_t s);   // depthwise_walk.hip

// DwpArgs / DwqArgs begin with the map's fields and end with `part`, the launch's geometry between them: the kernels' parameter
// types stay whole (their names are in the kernels' symbols, their offsets in the compiled text), the map is copied in by name.
template <class A>
static inline A dw_args_of(const DwMap& m) {
    A a;
    a.in = m.in; a.w = m.w; a.scale = m.scale; a.shift = m.shift; a.out = m.out;
    a.B = m.B; a.H = m.H; a.W = m.W; a.C8 = m.C8;
    a.ld_in = m.ld_in; a.ld_w = m.ld_w; a.ld_out = m.ld_out;
    a.pad_t = m.pad_t; a.pad_l = m.pad_l; a.act = m.act;
    a.part = m.part; a.ld_part = m.ld_part;
    return a;
}
// fn<yr_bf16 | yr_f16>(args...) for the map's element type (`form`: the name in the error message)
#define DW_BY_16(dt, form, fn, ...)                  \
    ((dt) == YR_BF16 ? fn<yr_bf16>(__VA_ARGS__)      \
     : (dt) == YR_F16 ? fn<yr_f16>(__VA_ARGS__)      \
                      : (yr_set_error("depthwise (" form " form): 16-bit maps only"), (int)YR_ERR_ARG))
// GO(ACT) for the op's activation - ACT: 0 ReLU6, 1 swish, 2 whatever a.act says (dw_act).  A launcher defines GO as the YR_LAUNCH of
// its kernel with ACT among the template arguments.  No launch of the family takes more than 64 KB of LDS and none raises the
// kernel's dynamic limit: they pass lds_max = 0.
#define DW_BY_ACT(act, GO) ((act) == YR_ACT_RELU6 ? GO(0) : (act) == YR_ACT_SWISH ? GO(1) : GO(2))

// ---------------------------------------------------------------- device side
typedef float dw_f2 __attribute__((ext_vector_type(2)));

// a 16-bit channel pair (one LDS word) -> float32, exact
template <class T>
__device__ __forceinline__ dw_f2 dw_widen(unsigned v) {
    typedef T t2 __attribute__((ext_vector_type(2)));
    return __builtin_convertvector(__builtin_bit_cast(t2, v), dw_f2);
}

// ACT: 0 ReLU6, 1 swish (the fast form of 16-bit stores, yr_apply_act_t), 2 whatever a.act says (a switch per value)
template <int ACT, class T>
__device__ __forceinline__ float dw_act(float v, int act) {
    if constexpr (ACT == 0) return yr_relu6_fast(v);
    else if constexpr (ACT == 1) return yr_swish_fast(v);
    else return yr_apply_act_t<T>(v, act);
}

// Loads and stores go through buffer descriptors over one image of the map, or the images of a workgroup (< 1 GB): a lane whose
// pixel is padding, whose channels are beyond C or whose column is beyond W passes an offset beyond num_records - the load returns
// zeros (the DMA writes zeros), the store is dropped - so neither needs clamped coordinates, selects or a per-lane branch.  Stores
// do not use YR_DEAD: a store's offset is a row part (dead, or < 2^30) plus a pixel part (dead, or < 2^30), either may be dead, and
// the sum must not wrap back into the map.
constexpr unsigned DW_LDEAD = 0x80000000u;   // load offsets
constexpr unsigned DW_SDEAD = 0x40000000u;   // store offsets: each part; a sum of two is at most 2^31

// One tap - column kx of the kernel, weight pair wt - over the four columns of a strip, into the partial sums of output row r.  An
// output row's first tap starts its sum from a literal zero.  The loops over (ky, kx) around it are the kernels' instruction order
// and stay with them.  (The arrays whole, not a row of acc or a pointer into col: those forms compile dwp_kernel to other text.)
template <int K, int NC>
__device__ __forceinline__ void dw_tap4(dw_f2 (&acc)[K][4], int r, const dw_f2 (&col)[NC], int kx, dw_f2 wt, bool first) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[r][i] = __builtin_elementwise_fma(col[i + kx], wt, first ? (dw_f2){0.f, 0.f} : acc[r][i]);
}

// The row read-ahead: a lane's NC = 4 + HALO words of an LDS row (pixels are 32 words apart), read one row AHEAD - raw holds the
// next input row, its reads issued under the taps of this one - and widened into col when its turn comes.
template <int NC>
__device__ __forceinline__ void dw_row_read(unsigned (&raw)[NC], const unsigned* p) {
#pragma unroll
    for (int c = 0; c < NC; ++c) raw[c] = p[c * 32];
}
template <class T, int NEXT, int NC>   // NEXT: the row to read ahead, counted from `rows`; 0: none, the last row's turn
__device__ __forceinline__ void dw_row_next(dw_f2 (&col)[NC], unsigned (&raw)[NC], const unsigned* rows, int pitch) {
#pragma unroll
    for (int c = 0; c < NC; ++c) col[c] = dw_widen<T>(raw[c]);
    if constexpr (NEXT > 0) dw_row_read(raw, rows + NEXT * pitch);
}

// The finish of an output row's four columns: BatchNorm, activation, ONE rounding to T, the store - at vector offset vrow + ooff[i]
// and scalar offset srow: the row reaches it either way - and, SE, the sum of what was stored (the rounded values).
template <class T, int ACT, bool SE>
__device__ __forceinline__ void dw_finish_row(const dw_f2 (&acc)[4], dw_f2 sc, dw_f2 sh, int act, yr_rsrc dst, const unsigned (&ooff)[4], unsigned vrow,
                                              unsigned srow, dw_f2& psum) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        typedef T t2 __attribute__((ext_vector_type(2)));
        const dw_f2 y = __builtin_elementwise_fma(acc[i], sc, sh);
        const t2 r = __builtin_convertvector((dw_f2){dw_act<ACT, T>(y.x, act), dw_act<ACT, T>(y.y, act)}, t2);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, r), dst, vrow + ooff[i], srow, 0);
        if constexpr (SE) psum += vrow + ooff[i] < DW_SDEAD ? __builtin_convertvector(r, dw_f2) : (dw_f2){0.f, 0.f};
    }
}
