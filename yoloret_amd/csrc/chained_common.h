// What the register-chained block kernels share, each rule stated once (float32: mbr.hip, mbk.hip, headwalk.hip, headstream.hip
// through mbr_common.h; 16-bit: mbxr_h.hip, headwalk_h.hip): the generator of the DPP depthwise tap group, the row-segment rule
// of the row-walking launchers and the tail of a template launcher.
#pragma once
#include "yr_common.h"

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));

// ---- THE DPP TAP GROUP.  After the expand MFMA a lane holds 4 consecutive channels of one pixel and the 16 lanes of a DPP row
// hold the strip's 16 pixels: a horizontal depthwise tap is one multiply-add per channel whose pixel operand is read through a
// DPP row shift, and a tap ROW is a few such groups in one asm statement.
//   * The shift rides on the multiply-add's first operand (v_fmac_f32_dpp: no v_mov_dpp, no extra register).  hipcc 7.2 does
//     not fold update_dpp into the fma (left to itself: 6 v_mov_b32_dpp + hazard nops per channel, one chain after the other).
//   * The four channels' chains are interleaved tap-major (a group = the four channels of ONE tap), so a dependent instruction
//     sits four slots behind its producer.
//   * "s_nop 1" in front of a statement whose row was just written: a VALU write must be two wait states ahead of a DPP read
//     of the same register, and the hazard recogniser does not look into asm.  Statements that read rows written long before
//     (mbk_dw_part: slices ago, or from LDS) carry none.
//   * An asm statement takes at most 30 operands: a five-tap row is two statements (taps 0..2, taps 3..4).
//   * (A packed form - v_pk_fma_f32 on row_shr / row_shl copies made once per row, scatter order - needs 26 instead of 36 VALU
//     slots per tile row, but its register tuples made hipcc 7.2 spill 100-600 bytes per lane on the stride-1 kernels: measured
//     slower everywhere it spilled, equal elsewhere.)
// Statement boundaries and operand lists decide scheduling and register allocation: the sites below keep theirs, operands a
// statement does not read included; tools/kernel_signature.py shows any change to the code that comes out.
//
// CH_TAP4(op, d, x, y, mods): the group - `op d[i], x[i], y[i] mods` for i = 0..3, DPP (if any) on x.  d, x, y name operand
// quadruples of the statement (%[d0] .. %[d3]), declared in its operand lists with CH_ACC4 / CH_OUT4 / CH_IN4.
#define CH_TAP1(op, d, x, y, i, mods) op " %[" #d #i "], %[" #x #i "], %[" #y #i "]" mods "\n\t"
#define CH_TAP4(op, d, x, y, mods) CH_TAP1(op, d, x, y, 0, mods) CH_TAP1(op, d, x, y, 1, mods) CH_TAP1(op, d, x, y, 2, mods) CH_TAP1(op, d, x, y, 3, mods)
#define CH_ACC4(n, v) [n##0] "+v"(v##0), [n##1] "+v"(v##1), [n##2] "+v"(v##2), [n##3] "+v"(v##3)                  // the scalars v0 .. v3, read and written
#define CH_OUT4(c, n, v) [n##0] c((v)[0]), [n##1] c((v)[1]), [n##2] c((v)[2]), [n##3] c((v)[3])                    // v[0 .. 3] under output constraint c
#define CH_IN4(n, v) [n##0] "v"((v)[0]), [n##1] "v"((v)[1]), [n##2] "v"((v)[2]), [n##3] "v"((v)[3])                // v[0 .. 3], read
// the modifiers: a row shift or permutation (lanes it shifts in from outside the row read 0), all banks or `bank` only written;
// row_newbcast: lane `lane` of the row, to the whole row (gfx90a+; tools/dpp_bcast_test.hip)
#define CH_DPP(ctl) " " ctl " row_mask:0xf bank_mask:0xf bound_ctrl:1"
#define CH_DPPM(ctl, bank) " " ctl " row_mask:0xf bank_mask:" bank " bound_ctrl:1"
#define CH_BCAST(lane, bank) " row_newbcast:" #lane " row_mask:0xf bank_mask:" bank
#define CH_OWN "quad_perm:[0,1,2,3]"   // the lane's own value, as a DPP control (so that the bank mask applies)
// a tap of the accumulators a0 .. a3 (CH_ACC4(a, a)) on the row e (CH_IN4(e, e)): shifted, or the lane's own pixel
#define CH_FMAC_DPP(w, mods) CH_TAP4("v_fmac_f32_dpp", a, e, w, mods)
#define CH_FMAC(w) CH_TAP4("v_fmac_f32", a, e, w, "")
// three shifted taps w0 .. w2 (operands W0 .. W2) in one statement, on a row that was just written: the paired stride-2 forms
#define CH_PAIR3(c0, c1, c2, bank, W0, W1, W2)                                                                                   \
    asm("s_nop 1\n\t" CH_FMAC_DPP(w0, CH_DPPM(c0, bank)) CH_FMAC_DPP(w1, CH_DPPM(c1, bank)) CH_FMAC_DPP(w2, CH_DPPM(c2, bank))  \
        : CH_ACC4(a, a) : CH_IN4(e, e), CH_IN4(w0, W0), CH_IN4(w1, W1), CH_IN4(w2, W2))

// ---- THE ROW-SEGMENT RULE of the row-walking launchers (launch_mbr, launch_mbe, launch_mbxr, launch_mbhr, launch_mbhq): a strip
// of Ho output rows is cut into segments so that about `target_waves` waves run (~2 or 3 per SIMD of the chip: 2 x 1024 for the
// workgroup forms, 3 x 1024 for the one-wave forms) - `walks` walks of `nw` waves each per segment -, but no segment shorter than
// `min_rows` rows (every segment recomputes its halo rows); want_segs > 0 (the tuner, a test) overrides that choice; `pairs`: the
// form walks pairs of output rows, a segment is an even number of rows.  Returns the rows of a segment, *segs = how many there
// are.  The tuner and the batch-invariance guarantee rest on this being ONE function of (shape, want_segs).
static inline int ch_row_segments(int Ho, int walks, int nw, int target_waves, int min_rows, bool pairs, int want_segs, int* segs) {
    int n = (target_waves + walks * nw - 1) / (walks * nw);
    const int max_segs = (Ho + min_rows - 1) / min_rows;
    if (n > max_segs) n = max_segs;
    if (n < 1) n = 1;
    if (want_segs > 0) n = want_segs < Ho ? want_segs : Ho;
    int seg_rows = (Ho + n - 1) / n;
    if (pairs) seg_rows += seg_rows & 1;
    *segs = (Ho + seg_rows - 1) / seg_rows;
    return seg_rows;
}

#ifdef __HIPCC__
// ---- THE LAUNCH TAIL of a template launcher is yr_launch (yr_common.h); here with the kernel's name formatted once per instantiation
// from name_fmt, whose arguments are its template parameters.
template <auto KERN, class Args, class... NameArgs>
static int ch_launch(dim3 grid, dim3 block, size_t lds, size_t lds_max, hipStream_t s, const Args& a, const char* name_fmt, NameArgs... name_args) {
    static const yr_kname nm = yr_kname_fmt(name_fmt, name_args...);
    return yr_launch<KERN>(nm.s, grid, block, lds, lds_max, s, a);
}
#endif
