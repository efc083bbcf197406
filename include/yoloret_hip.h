/* yoloret_hip.h - C-ABI of libyoloret_hip.so: the MI355X (gfx950) detection-forward
 * runtime behind yoloret_amd's Python surface.
 *
 * The reference (prakharg24/yoloret) has NO native / FFI interface: its path is
 * Python calling TensorFlow kernels.  Each entry point below therefore cites
 * the reference Python function (file:line under /root/reference/code) whose TF
 * kernels it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - all tensors NHWC.  Element type (yr_dtype): float32, or - activations between the ops of a
 *     reduced-precision plan (BASELINE.json configs 3 and 5) - bfloat16 / float16.  Images in, the
 *     three logit outputs, BatchNorm scale/shift, depthwise weights, SE vectors and everything
 *     behind the logits (decode, NMS) are float32 in every plan; all accumulation is float32.
 *   - `ld` = channel stride in ELEMENTS (>= channels; a multiple of 4 for float32 tensors and of 8
 *     for 16-bit tensors unless stated, i.e. every pixel row is 16-byte aligned); every device
 *     pointer 16-byte aligned.
 *   - every function returns 0 on success, a negative yr_status otherwise, and
 *     never throws; the message is available from yr_last_error().
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it
 *     asynchronously, nothing synchronises.
 *   - a handle is bound to the device that was current at yr_create and is not
 *     thread-safe.
 */
#ifndef YOLORET_HIP_H
#define YOLORET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YR_ABI_VERSION 9   /* 9: float32 POINTWISE se_reduced bit 18 = the pixel-stationary form (pointwise_stream.hip: `wgt` holds the weights' float16 planes in fragment order) and bit 19 = its two-output form (gate_out / se_hidden / reserved0 = a second conv of the same source); plans of ABI 8 run unchanged - only the version word of a serialised plan differs; 8: YR_OP_MBR k bit 6 = the weight-streaming form of the fused block (mbk.hip; plans of ABI 7 run unchanged - only the version word of a serialised plan differs); 7: squeeze-excite finished by its producer (yr_op.gate_out / se_w / se_hidden / sync: the "SE tail"), op kind HEAD (gathered 1x1 conv -> depthwise 3x3 -> SE of a detection-head block in one launch), yr_workspace_bytes includes the arrival counters; 6: split forms - k bit 7 of MBR / MBE (float16-plane fragments), se_reduced bit 16 of a float32 POINTWISE op (= keep the float32 MFMA); float32 POINTWISE ops at least 16 channels deep otherwise run on the 16-bit matrix pipe with two float16 planes per operand (pointwise_split.hip; same results to float32 rounding, |x|, |w| < 65504); 5: op kinds MBR / MBE (float32 blocks on the matrix pipe, register-chained), MBCONV removed; 4: YR_U8 images (uint8 network entry); 3: op kind MBX, pair-packed STEM weights, BN scale folded into the packed taps of STEMBLOCK / MBLANE */
#define YR_MAX_SRC 4

typedef enum {
    YR_OK = 0,
    YR_ERR_ARG = -1,     /* bad argument / unsupported shape */
    YR_ERR_HIP = -2,     /* a HIP runtime call failed */
    YR_ERR_STATE = -3    /* e.g. weights not loaded */
} yr_status;

/* Element type of an activation tensor / of the POINTWISE weight matrix.  The 16-bit types are storage formats:
 * every kernel converts to float32 on load (bf16: exact widening) and rounds to nearest-even on store; only the
 * POINTWISE GEMM consumes them natively (v_mfma_f32_16x16x32_bf16 / _f16, float32 accumulate). */
typedef enum { YR_F32 = 0, YR_BF16 = 1, YR_F16 = 2,
               YR_U8 = 3   /* ABI 4: uint8 - ONLY as the element type of the image (external slot 0) read by a STEM / STEMBLOCK op: the
                              decoded bytes as they are, x / 255 (code/yolo.py:106) applied inside the kernel; the float32 batch
                              (4x the bytes) is then never written or read */
} yr_dtype;

typedef enum { YR_ACT_NONE = 0, YR_ACT_RELU6 = 1, YR_ACT_SWISH = 2, YR_ACT_SIGMOID = 3, YR_ACT_LEAKY = 4 } yr_act;

/* How a source tensor is read by a consumer (folds Keras UpSampling2D /
 * MaxPooling2D / Concatenate - model.py:139-144,157,164-166,253-255,307-308 -
 * into the consumer's loads). */
typedef enum {
    YR_X_IDENTITY = 0, YR_X_UP2 = 1, YR_X_MAXPOOL2 = 2, YR_X_MAXPOOL4 = 3,
    /* POINTWISE only, last source only: NOT part of the k space.  Its `cout` channels, gathered with nearest 2x
     * upsampling, are added to the accumulator before BatchNorm.  A 1x1 convolution commutes with nearest
     * upsampling (W.[up2(a); b] = up2(Wa.a) + Wb.b), so the compiler computes the upsampled share of a concat conv
     * at the source resolution and hands it in this way (model.py:253-255,273-275: UpSampling2D + Concatenate feeding
     * the first 1x1 conv of the top-down heads). */
    YR_X_UP2_ADD = 4,
    /* POINTWISE only, the single source: the source is read THROUGH DepthwiseConv2D 3x3 (TF 'SAME') + BatchNorm +
     * activation, i.e. the conv's input channel k at an output pixel is act(BN(sum over the 3x3 taps of
     * dw_w[tap][k] * src[pixel*stride + tap][k])) - the depthwise stage of an inverted-residual block folded into
     * the loads of its projection (MobileNetV2 block_* [3P] depthwise + project; efficientnet.py:501-533).  The
     * depthwise result (the block's widest tensor besides the expand output) never reaches HBM; values are
     * bit-identical to a DEPTHWISE op followed by the same POINTWISE op.  Op fields: src[0] = the depthwise INPUT
     * (its h, w), op.h/op.w = the depthwise OUTPUT dims, se_reduced = stride | (yr_act of the depthwise stage << YR_PWDW_ACT_SHIFT),
     * wgt2 = depthwise weights [9][ld], b1 / b2 = its folded BN scale / shift [ld], ld = round_up(src.c, 4). */
    YR_X_DW3 = 5
} yr_xform;

/* One concatenated input segment.  (h,w) are the SOURCE's spatial dims; the
 * consumer's dims follow from xform.  In plan ops `ptr` is unused and `buf`
 * indexes the plan's buffer table; in yr_op_* calls `ptr` is the device pointer. */
typedef struct {
    const void* ptr;
    int32_t buf;
    int32_t h, w;
    int32_t c;       /* channels taken from this source */
    int32_t ld;      /* channel stride of the source buffer, in elements */
    int32_t xform;   /* yr_xform */
    int32_t dtype;   /* yr_dtype of the source buffer: must equal the op's `dtype`, except for sources that are float32
                        in every plan (the image of STEM / STEMBLOCK, a YR_X_UP2_ADD source, the pooled vector of SE_FC) */
} yr_src;

typedef enum {
    YR_OP_STEM = 1,      /* Conv2D 3x3 s2 Cin=3 + BN + act            (MobileNetV2 Conv1 [3P]; efficientnet.py:636-645).  Optional
                            wgt2 = the same parameters packed per channel PAIR, [round_up(cout,4)/2][27 taps x 2, times the BN
                            scale | 1 1 | BN shift 2] (STEMBLOCK's stem layout): selects the scalar-operand kernel */
    YR_OP_POINTWISE = 2, /* Conv2D 1x1 (+bias)(+BN)(+act)(+residual)  (model.py:25-30,98-114,152-155,243-251; efficientnet.py:485-496,517-533)
                            se_reduced flags YR_PWF_* (no depthwise-folded source): float32 ops, YR_PWF_F32_MFMA = keep the float32 MFMA (not the
                            float16-plane split form); YR_PWF_KSPLIT (round 5, no layout change) = the k-split form of the split kernel - a
                            workgroup is one 16 x 16 output tile, its four waves split the k range (pointwise_split.hip: pwk_kernel; 16-bit ops:
                            one 16 x 32 tile, pointwise_h.hip: pwkh_kernel);
                            what the compiler's plan for one or two images asks of maps up to 32 x 32.  The form groups the sums by wave: it
                            belongs to the plan, not to the tuner (yr_op.k is not looked at); ignored below 64 input channels.
                            YR_PWF_STATIONARY (ABI 9, float32 ops without YR_PWF_F32_MFMA / YR_PWF_KSPLIT; identity | up2 sources, no residual / up2_add, act none | ReLU6,
                            k space <= 384 channels): the PIXEL-STATIONARY form (pointwise_stream.hip) - `wgt` is NOT Wt[cout][kp] but its float16
                            planes in MFMA fragment order, [ceil(cout / 16)][NK][2 planes h | m][64 lanes][8 halves] as float32 words with
                            NK = yr_pwt_chunks(kp) chunks of 32 channels (lane (m, g) of tile t, chunk c: W[16 t + m][32 c + 8 g + i], zero
                            beyond cout / kp; h = f16(w), m = f16((w - h) 2^11): compiler.head_pack).  Results are bit-identical to the tiled
                            split kernel's.  YR_PWF_TWO_OUT (with YR_PWF_STATIONARY): TWO outputs - a second 1x1 conv of the same (gated) single identity source in
                            the same launch: gate_out / gate_out_buf / gate_out_ld = its output (float32), se_hidden = its couts,
                            reserved0 = its yr_act | YR_PW2_POOLED (MaxPooling2D(2) of its result, like stride = 2 for the first); its cout tiles
                            follow the first output's in `wgt`, and scale / shift are [16 (tiles of the first + tiles of the second)]
                            floats, each output's values padded to a multiple of 16. */
    YR_OP_DEPTHWISE = 3, /* DepthwiseConv2D k3/k5 s1/s2 SAME + BN + act (model.py:20-24; efficientnet.py:501-510).  With `gate` set (SE
                            form): the kernel ALSO writes per-workgroup channel sums of its output to
                            gate = float32 [B][se_reduced rows][gate_ld] (rows: compiler.dw_se_geometry == depthwise.hip) - the squeeze of squeeze-excite (efficientnet.py:417) as an
                            epilogue; an SE_FC op with k = H*W adds the rows up instead of re-reading the map */
    YR_OP_SE_MEAN = 4,   /* Mean over H,W                              (efficientnet.py:391-403,417) */
    YR_OP_SE_FC = 5,     /* 1x1+bias -> Swish -> 1x1+bias -> sigmoid   (efficientnet.py:419-434).  Source: the pooled vector (h*w == 1,
                            float32), or a map to pool first (SE_MEAN merged in), or - k > 0 - float32 rows of partial channel
                            sums [B][h*w][ld] to add up and divide by k (the depthwise SE form above) */
    YR_OP_WSUM = 6,      /* WeightedSum of 4 gathered sources          (model.py:117-137,157) */
    YR_OP_GATHER = 7,    /* materialise upsample/maxpool/concat        (standalone K5; testing / unfused use) */
    YR_OP_MBCONV = 8,    /* (removed in ABI 5: the float32 LDS-tiled block kernel; no shipped plan selected it since MBLANE, and MBR / MBE
                            now take the blocks it was the fallback for.  The number stays reserved; yr_op_run returns YR_ERR_ARG) */
    YR_OP_STEMBLOCK = 9, /* fused network entry: stem Conv2D 3x3 s2 (Cin=3)+BN+act -> DW3x3 s1+BN+act -> project 1x1+BN
                            (MobileNetV2 Conv1 + expanded_conv block [3P]); se_reduced = stem width C1.  Parameters are packed
                            per channel PAIR (CP = round_up(C1,4)/2, COP = round_up(cout,8), zero padded; scale/shift unused):
                            wgt  = stem      [CP][27 taps (ky,kx,ci) x 2, times the BN scale | 1 1 | BN shift 2],
                            wgt2 = depthwise [CP][ 9 taps (ky,kx)    x 2, times the BN scale | 1 1 | BN shift 2],
                            b1   = project W[2*CP][COP] (input-channel major), b2 = project BN scale[COP] ++ shift[COP].
                            Built for (CP,COP) in {(12,16),(16,16),(16,24),(20,24),(24,16),(24,24)}; others: YR_ERR_ARG.
                            Without b1 (no projection; cout == C1, CP in {16,20,24}): stem + depthwise only - the depthwise
                            map is stored and, if `gate` is set, gate = OUTPUT float32 [B][ceil(h/14)*ceil(w/14)][gate_ld]
                            per-tile channel sums of the stored values (the squeeze of the first SE block).
                            MATRIX-PIPE LAYOUT (16-bit plans, round 3; selected by scale != NULL; C1 <= 64, cout <= 32, even image
                            sizes; C1P = round_up(C1,32), COP = round_up(cout,16), zero padded; stemblock_h.hip):
                            wgt = stem kernel as dtype [C1P][32], k order: image rows 0..2 x values 0..7 of the row's 9 (kx,ci) |
                            value 8 of rows 0..2 | 0 x 5;  scale / shift = stem BN [C1P];  wgt2 = float32 [10][C1P]: nine depthwise
                            taps times the BN scale | BN shift;  b1 = project Wt[COP][C1P] as dtype;  b2 = project BN [2][COP] */
    YR_OP_MBH = 11,      /* the MBCONV block on 16-bit activations, both 1x1 convs on bf16 / f16 MFMA, depthwise K = 3 | 5 from an
                            LDS tile (dtype must be YR_BF16 / YR_F16; cin, cout <= 128).  se_reduced = Cexp; k = K, optionally
                            | th << YR_MBH_TH_SHIFT | tw << YR_MBH_TW_SHIFT to force the output tile.  CexpP = round_up(Cexp,32), KP = round_up(cin,32),
                            zero padded: wgt = expand Wt[CexpP][KP] (16-bit); wgt2 = [K*K + 4][CexpP] float32: depthwise taps |
                            depthwise BN scale | shift | expand BN scale | shift;
                            b1 = project Wt[cout][CexpP] (16-bit); b2 = project BN scale ++ shift, [round_up(cout,8)] each;
                            res (optional) = the block input (stride 1, cin == cout).  The library runs K = 3, stride 2, cin <= 32
                            (cin % 8 == 0), Cexp <= 192, cout <= 32, no residual, no forced tile on mbn_h.hip (whole expanded
                            halo tile on chip in the 16-bit type: same op fields) */
    YR_OP_MBLANE = 10,   /* the MBCONV block (same layers, same op fields) in the lane-per-pixel formulation for narrow
                            block inputs (Cin <= 32): packed-fp32 FMA with scalar-register weights instead of MFMA.
                            se_reduced = Cexp; parameters packed per expanded-channel PAIR, P = round_up(ceil(Cexp/2),8),
                            CINP = round_up(Cin,4), COP = round_up(cout,8), zero padded; scale/shift unused:
                            wgt  = expand    [P][CINP x 2 (input-channel major), times the BN scale | 1 1 | BN shift 2],
                            wgt2 = depthwise [P][9 taps (ky,kx) x 2, times the BN scale | 1 1 | BN shift 2],
                            b1   = project W[2P][COP] (expanded-channel major), b2 = project BN scale[COP] ++ shift[COP].
                            Built for (CINP/4,COP) in {(4,16),(4,24),(6,24),(6,32),(6,40),(6,48),(8,32),(8,40),(8,48)}.
                            wgt = NULL: a block WITHOUT expand conv (expand ratio 1, efficientnet.py:467 skipped; stride 1,
                            se_reduced = Cin): depthwise + project (+ residual) on the block input itself; built for
                            (4,16), (6,24), (8,32) */
    YR_OP_MBR = 13,      /* the MBCONV block (same layers) in float32 on the fp32 matrix pipe, ROW-WALKING and REGISTER-CHAINED
                            (mbr.hip): a wave walks a strip of 16 input columns row by row; expand GEMM (v_mfma_f32_16x16x4_f32, the
                            strip row's pixels as N, block input straight from global memory in operand layout) -> the MFMA result
                            registers ARE the depthwise conv's input (horizontal taps by DPP, vertical taps = the last three rows kept
                            in registers) -> the depthwise result registers ARE the projection MFMAs' B operand.  The expanded tensor
                            never leaves the register file; the waves of a workgroup split the expanded channels and add their partial
                            projections through LDS.  dtype = YR_F32; act = YR_ACT_RELU6; cin % 16 in {0, 8}; se_reduced = Cexp, a
                            multiple of 16; cout % 4 == 0; k = 3 | nw << YR_MBR_NW_SHIFT | segs << YR_MBR_SEGS_SHIFT (nw: waves per workgroup, segs: row segments
                            per strip; 0 = the library's choice); res (optional) = the block input.  T = Cexp / 16 expanded tiles,
                            TO = ceil(cout / 16), KE = cin / 4 expand steps; scale / shift / b1 unused:
                            wgt  = MFMA A fragments [T][KE + 4 TO][64 lanes]; register rho of lane l (m = l % 16, g = l / 16) of tile j:
                                   rho < KE: We[16 j + m][kperm(rho, g)] x expand BN scale, kperm(4 c + s, g) = 16 c + 4 g + s for the full
                                   16-channel chunks of cin and 16 n + 2 g + s (s < 2) for a trailing 8;
                                   rho = KE + 4 t + s: Wp[16 t + m][16 j + 4 g + s] x project BN scale (0 for 16 t + m >= cout);
                            wgt2 = [T][11][16]: the nine depthwise taps (ky, kx) x depthwise BN scale | depthwise BN shift | expand BN shift;
                            b2   = project BN shift [16 TO].
                            k & YR_MBR_SPLIT = the SPLIT form (ABI 6): both 1x1 convolutions on the 16-bit matrix pipe with float32-grade operands -
                            every float32 value as two float16 planes, x = h + 2^-11 m, three MFMAs per product (mbr.hip "SPLIT form") -; then
                            wgt  = the float32 words holding [T][ceil(cin / 32)][2 planes][64 lanes][8 halves] (lane (m, g), step c:
                                   We[16 j + m][32 c + 8 g + i] x BN scale, zero beyond cin) followed by, per expanded-tile pair (tA, tB) of the nw
                                   waves in order (a wave pairs ITS tiles, an odd last one with nothing), [TO][2 planes][64][8]:
                                   Wp[16 t + m][16 tA + 4 g + i] (i < 4) | Wp[16 t + m][16 tB + 4 g + i - 4]; nw must be what the fragments were
                                   packed for (yoloret_amd.compiler.mbs_pack).  Precondition: |block input| < 65504 (undefined beyond: NaN or a ReLU6-clamped value).
                            k & (YR_MBR_STREAM | YR_MBR_SPLIT), both = the WEIGHT-STREAMING form (ABI 8; mbk.hip): the same block in ONE launch where the fragments of both
                            convolutions do not fit a CU's register file (MobileNetV2 x0.75 block_7..15, reference [3P] via code/yolo3/override.py:290-341).
                            The pixels are stationary - a wave owns `rows` (1 | 2) input rows of a 16-column strip and the projection accumulators of
                            its output rows for the whole kernel - and the weights stream through LDS one pair of expanded tiles at a time (LDS-direct
                            buffer loads, three chunk buffers); the neighbour rows of the vertical taps are exchanged between waves through LDS, one
                            barrier per pair.  k = 3 | YR_MBR_STREAM | YR_MBR_SPLIT | nw << YR_MBR_NW_SHIFT | rows << YR_MBR_SEGS_SHIFT (both fixed by the plan: nothing is tuned, the sums are grouped by
                            the shape alone); wgt2 unused;
                            wgt  = ceil(T / 2) chunks of (4 ceil(cin / 32) + 2 TO) KB + 2 KB: chunk q = pair (2 q, 2 q + 1) =
                                   [2 tiles][ceil(cin / 32)][2 planes][64 lanes][8 halves] expand fragments (as above) |
                                   [TO][2 planes][64][8] project fragments of the pair (Wp[16 t + m][16 (2 q) + 4 g + i] (i < 4) | [16 (2 q + 1) + 4 g + i - 4]) |
                                   [2 tiles][11][16] float32: taps x depthwise BN scale | depthwise BN shift | expand BN shift | zeros up to 2 KB
                                   (an odd T: the second tile of the last pair is all zeros) - yoloret_amd.compiler.mbk_pack;
                            b2   = project BN shift [16 TO].  Same precondition as the split form.  Built for (cin, Cexp, cout, stride, rows, nw) in
                            mbk.hip's MBK_CASE list.
                            Built for the MobileNetV2 x0.75 / x1.4 blocks (mbr.hip: MBR_CASE / MBS_CASE lists); other shapes: YR_ERR_ARG */
    YR_OP_MBE = 14,      /* the first two thirds of the MBCONV block in float32 - expand 1x1 + BN + ReLU6 -> depthwise 3x3 (stride 1 | 2) +
                            BN + ReLU6 - in YR_OP_MBR's register-chained form (mbr.hip: mbe_kernel), for blocks whose weights do not fit
                            one CU's register file (MobileNetV2 x0.75 block_11 on): every wave walks a strip segment for a few expanded
                            tiles and stores the depthwise map; the expand output never exists, the projection stays a POINTWISE op.
                            src[0] = block input (cin % 16 in {0, 8}); cout = Cexp (multiple of 16); k = 3 | segs << YR_MBR_SEGS_SHIFT; act = RELU6;
                            wgt = expand A fragments [T][KE][64] (YR_OP_MBR's register order, rho < KE); wgt2 = [T][11][16] as YR_OP_MBR.
                            k & YR_MBR_SPLIT = the split form (see YR_OP_MBR): wgt = the float32 words holding [T][ceil(cin / 32)][2 planes][64][8 halves].
                            Built for cin in {48, 72, 88, 120, 136, 224} (the split form: all but 224) */
    YR_OP_HEAD = 15,     /* ABI 7: the first two thirds of a detection-head block (model.py:91-115: Conv2D 1x1 + BN + ReLU6 -> MBConvBlock's
                            depthwise 3x3 + BN + Swish [-> SE]) in one launch, float32 (headblock.hip): the 1x1 convolution as YR_OP_POINTWISE's
                            split form (same sources incl. up-sampling / pooling / concat gathers, a YR_X_UP2_ADD last source, an SE `gate` on a
                            single identity source; operands as two float16 planes, |x|, |w| < 65504) over a REGION of one image with its
                            one-pixel halo, the F-wide conv output kept in LDS, the depthwise conv (stride 1, TF SAME) computed from there,
                            stored, and - with the SE-tail fields below - summed per channel.  The F-wide conv output never reaches HBM.
                            h, w = the map (conv and depthwise output alike); cin = sum of src[].c; cout = F; act = the depthwise activation;
                            k = 3 | conv activation << YR_HEAD_ACT_SHIFT; stride = 1; wgt = Wt[F][kp], scale / shift [F] (conv BN) as POINTWISE;
                            k & YR_HEAD_PLANES: wgt = the float32 words holding float16 planes in fragment order instead,
                            [ceil(F / 16)][NK][2 planes][64 lanes][8 halves] with the k space cut into chunks of 32 channels PER SOURCE (NK =
                            sum of ceil(src.c / 32); lane (m = l % 16, g = l / 16) of cout tile t, chunk j of source s: W[16 t + m][channel
                            32 j + 8 g + i of s], zero beyond the source / beyond F; h plane, then m = f16((w - h) 2^11)) - the LDS-direct
                            kernel (identity / up-sampled sources only; yoloret_amd.compiler.head_pack);
                            wgt2 = float32 [10][round_up(F, 4)]: the nine depthwise taps (ky, kx) x depthwise BN scale | depthwise BN shift.
                            k & YR_HEAD_WALK: the WALKING form (headwalk.hip: a wave walks a strip of 16 columns with the weights of its cout tiles
                            in registers - YR_OP_MBE's scheme; identity sources only, at most 7 chunks of 32 channels, F % 16 == 0, conv
                            activation ReLU6 / none): wgt = the planes of YR_HEAD_PLANES WITH the conv's BN scale folded in, scale = that BN scale [F],
                            shift unused, wgt2 = [F / 16][11][16]: depthwise taps x BN scale | depthwise BN shift | conv BN shift (YR_OP_MBR's
                            table); se_reduced = yr_head_walk_rows(h, w).
                            (k & YR_HEAD_STREAM) == YR_HEAD_STREAM (ABI 8): the WEIGHT-STREAMING form (headstream.hip; float32 plans): the pixels of a wave's one or two
                            rows of a 16-column strip stay in registers over the whole k space (gathered once: identity or 2 x 2 max-pooled
                            sources, the single source's SE gate), the conv's output channels stream past them in pairs of tiles through LDS.
                            Parameters exactly as YR_HEAD_WALK alone; one to three k-space sources (YR_X_IDENTITY | YR_X_MAXPOOL2) + an optional
                            YR_X_UP2_ADD last; at most 11 chunks of 32 channels on maps below 20 rows, 7 otherwise; F % 32 == 0; no SE tail;
                            se_reduced = yr_head_stream_rows(h, w) (one row of sums per strip, row segment and wave).
                            16-BIT PLANS (dtype = out_dtype = bf16 | f16; headwalk_h.hip): the walking form only (YR_HEAD_WALK) - identity sources
                            of the op's type (ld % 8 == 0), optionally a float32 YR_X_UP2_ADD last source, at most 8 chunks of 32 channels,
                            F % 128 == 0; wgt = the conv's 16-bit weights in fragment order [F / 16][NK][64 lanes][8] WITHOUT the BN scale
                            (yoloret_amd.compiler.head_pack16), scale = conv BN scale [F] float32, wgt2 as above; float32 from the
                            accumulator on, ONE rounding at the store (the F-wide conv output is never rounded to 16 bits), the sums are
                            those of the stored values; an SE gate (res) is folded into the stationary weights (w * g rounded once);
                            no SE tail (gate_out must be null).
                            res / res_ld (optional) = the float32 SE gate vector [B][res_ld] multiplied onto the single identity source on load
                            (`gate` is taken by the sums this op writes); k & YR_HEAD_TILES_MASK (optional) = cout tiles of 16 per workgroup.
                            SE tail: gate = OUTPUT float32 [B][se_reduced][gate_ld] channel sums, one row per region (se_reduced = regions per
                            image: yr_head_regions()) */
    YR_OP_MBX = 12       /* the first two thirds of an MBConv block WITH squeeze-excite (efficientnet.py:406-536), 16-bit
                            activations: expand 1x1 + BN + act (bf16 / f16 MFMA) -> depthwise K = 3 | 5, stride 1 | 2 + BN +
                            act, the expanded input of the depthwise conv staying in LDS; the depthwise map is stored and
                            the squeeze (tf.reduce_mean over H, W, efficientnet.py:417) leaves as per-tile channel sums.
                            src[0] = block input (cin <= 128); cout = Cexp = width of the stored map; wgt, wgt2, k as MBH;
                            gate (optional) = OUTPUT float32 [B][se_reduced][gate_ld] sums of the STORED values, one row
                            per output tile, unused rows zeroed (se_reduced = rows >= tiles per image: the buffer is sized
                            for the smallest tile the host may pick, 4 x 8, or 4 x 4 on maps under 1000 pixels); SE_FC (k = H*W) adds the rows up; the projection stays a POINTWISE op */
} yr_op_kind;

/* ---- LAUNCH-FORM BITS: every sub-field and flag that is packed into yr_op.k, yr_op.se_reduced and yr_op.reserved0, per op kind.
 * (yoloret_amd/runtime.py mirrors this block name by name, without the YR_ prefix; tests/test_host_logic.py compares the two.)
 * A name of one op kind means nothing on another: the same bit of `k` is a different form there.  A *_MASK selects its field in
 * place, the field's value is (x & *_MASK) >> *_SHIFT. */
/* YR_OP_POINTWISE, se_reduced of an op WITHOUT a depthwise-folded source (float32 ops unless stated): */
#define YR_PWF_F32_MFMA     0x10000    /* bit 16: keep the float32 MFMA (not the float16-plane split form) */
#define YR_PWF_KSPLIT       0x20000    /* bit 17: the k-split form of the split kernel (float32 and 16-bit ops) */
#define YR_PWF_STATIONARY   0x40000    /* bit 18: the pixel-stationary form - `wgt` holds float16 planes in fragment order */
#define YR_PWF_TWO_OUT      0x80000    /* bit 19 (with bit 18): two outputs */
/* YR_OP_POINTWISE, se_reduced of an op WITH a YR_X_DW3 source = the depthwise stage's stride | its yr_act << 8: */
#define YR_PWDW_STRIDE_MASK 0xff
#define YR_PWDW_ACT_SHIFT   8
#define YR_PWDW_ACT_MASK    0xff00
/* YR_OP_POINTWISE, reserved0 of a two-output op = the second output's yr_act | pooled flag: */
#define YR_PW2_ACT_MASK     0xff
#define YR_PW2_POOLED       0x100      /* bit 8: MaxPooling2D(2) of the second output's result */
/* YR_OP_MBR / YR_OP_MBE, k = kernel size | form flags | nw << 8 | segs (weight-streaming form: rows) << 16: */
#define YR_MBR_K_MASK       0x3f       /* the depthwise kernel size (3) */
#define YR_MBR_STREAM       0x40       /* bit 6 (MBR only, with YR_MBR_SPLIT): the weight-streaming form (mbk.hip) */
#define YR_MBR_SPLIT        0x80       /* bit 7: the split form - float16-plane fragments */
#define YR_MBR_FORM_MASK    0xff       /* kernel size and form flags: the byte that belongs to the plan, never to a tuning word */
#define YR_MBR_NW_SHIFT     8          /* waves per workgroup (0 = the library's choice) */
#define YR_MBR_NW_MASK      0xff00
#define YR_MBR_SEGS_SHIFT   16         /* row segments per strip (0 = the library's choice); weight-streaming form: rows per wave */
#define YR_MBR_SEGS_MASK    0xff0000
/* YR_OP_HEAD, k = kernel size | form flags | the conv's yr_act << 8 | cout tiles per workgroup << 16: */
#define YR_HEAD_K_MASK      0x1f       /* the depthwise kernel size (3) */
#define YR_HEAD_STREAM_BIT  0x20       /* bit 5: only together with YR_HEAD_WALK (= YR_HEAD_STREAM) */
#define YR_HEAD_WALK        0x40       /* bit 6: the walking form (headwalk.hip, headwalk_h.hip) */
#define YR_HEAD_PLANES      0x80       /* bit 7: `wgt` holds float16 planes in fragment order (the LDS-direct kernel) */
#define YR_HEAD_STREAM      (YR_HEAD_WALK | YR_HEAD_STREAM_BIT)   /* bits 5 and 6: the weight-streaming form (headstream.hip) */
#define YR_HEAD_ACT_SHIFT   8          /* yr_act of the 1x1 convolution (yr_op.act is the depthwise stage's) */
#define YR_HEAD_ACT_MASK    0xff00
#define YR_HEAD_TILES_SHIFT 16         /* cout tiles of 16 per workgroup (0 = the library's choice) */
#define YR_HEAD_TILES_MASK  0xff0000
/* YR_OP_MBH / YR_OP_MBX, k = kernel size | th << 8 | tw << 16 (the forced output tile; 0 = the library's choice): */
#define YR_MBH_K_MASK       0xff       /* the depthwise kernel size (3 | 5) */
#define YR_MBH_TH_SHIFT     8
#define YR_MBH_TH_MASK      0xff00
#define YR_MBH_TW_SHIFT     16
#define YR_MBH_TW_MASK      0xff0000
#define YR_MBH_TILE_LDS     254        /* th: force the LDS-tiled kernels' own choice (mbh.hip, mbn_h.hip), never the register-chained forms */
#define YR_MBH_TILE_CHAINED 255        /* th: force the register-chained kernel (mbxr_h.hip); tw = row segments */
/* YR_OP_STEMBLOCK, k = kernel size | entry form << 8: */
#define YR_STEMBLOCK_K_MASK      0xff
#define YR_STEMBLOCK_ENTRY_SHIFT 8
#define YR_STEMBLOCK_ENTRY_MASK  0xff00
#define YR_STEMBLOCK_ENTRY_MFMA  1     /* entry form: the matrix-pipe form of the stem + depthwise entry */
/* The tuning word of an op (yr_set_tuning / yr_get_tuning) uses the positions of that op kind's `k`: MBH / MBX th << YR_MBH_TH_SHIFT |
 * tw << YR_MBH_TW_SHIFT, MBR / MBE nw << YR_MBR_NW_SHIFT | segs << YR_MBR_SEGS_SHIFT, the low byte zero.
 * ---- end of the launch-form bits */

/* One fused operation.  Weight-like fields are float offsets into the weight
 * blob in plan ops (`wgt_off` etc.), or device pointers in yr_op_* calls.
 *
 * Where an op touches memory (tests/fence.py holds every op of the suite to this, between guard bytes):
 *   - it writes only the bytes of its outputs.  Of `out` (and of the second output of a two-output POINTWISE op) these are, per
 *     pixel row of out_ld elements, elements [0, round_up(cout, V)) - V = 4 for a float32 output, 8 for a 16-bit one - or
 *     [0, cout) where the row is dense (out_ld == cout); elements behind them, up to out_ld, keep what they held.  The other
 *     outputs are written whole, as sized at their fields: the channel-sum rows behind `gate` (B x se_reduced x gate_ld), the
 *     SE tail's gate_out (B x gate_out_ld), `sync` (B words, zero again after the launch), SE_MEAN's and SE_FC's `out` (B x out_ld);
 *   - no byte outside a source's B x h x w x ld elements (nor outside a gate's B x gate_ld, a residual's B x h x w x res_ld, a
 *     parameter array's documented extent) influences a result: a kernel may fetch a halo row, a k-tail quad or a pooled window
 *     past a tensor's end only if the value never reaches an output;
 *   - 16-byte alignment of every pointer suffices (4-byte where a field is documented as dwords: `sync`); nothing may rely on the
 *     larger alignment an allocator happens to give. */
typedef struct {
    int32_t kind;         /* yr_op_kind */
    int32_t act;          /* yr_act */
    int32_t h, w;         /* OUTPUT spatial dims per image */
    int32_t cin, cout;    /* logical channels (cin = sum of src[].c) */
    int32_t k, stride;    /* DEPTHWISE / STEM kernel size and stride */
    int32_t nsrc;
    int32_t se_reduced;   /* SE_FC: hidden width */
    int32_t dtype;        /* yr_dtype the op works in: element type of its sources, residual and (POINTWISE) `wgt`;
                             16-bit types: every op kind except MBCONV */
    int32_t out_dtype;    /* yr_dtype of `out`: equal to `dtype`, or YR_F32 from a 16-bit POINTWISE op (logit outputs,
                             the low-resolution partial sums of a hoisted conv); SE_MEAN / SE_FC always write float32 */
    yr_src src[YR_MAX_SRC];
    /* output */
    void* out;  int32_t out_buf;  int32_t out_ld;    /* out_ld may exceed the padded width (a multiple of V): the elements behind round_up(cout, V) are
                                                         left alone (tests: *_wide_rows).  Refused with YR_ERR_ARG: YR_OP_MBX in its LDS-tiled
                                                         form (mbh.hip: a forced tile, or a shape the register-chained form is not built for),
                                                         which needs out_ld == round_up(cout, 8); no other kind refuses a wider row */
    /* optional residual added after BN (same shape as output, element type `dtype`) */
    const void* res;  int32_t res_buf;  int32_t res_ld;
    /* optional SE gate [B, gate_ld] (float32) multiplied onto the (single) source on load */
    const float* gate;  int32_t gate_buf;  int32_t gate_ld;
    /* parameters (device pointers, or float offsets into the blob when in a plan); float32 unless stated:
     *   POINTWISE: wgt = Wt[cout][kp] of element type `dtype` (kp = sum of round_up(src.c, V), V = 4 for float32 and 8
     *              for the 16-bit types, zero padded; in the blob a 16-bit matrix occupies cout*kp/2 floats),
     *              scale/shift [cout] (folded BN and/or bias)
     *   DEPTHWISE: wgt = [k*k][round_up(c,V)] ; scale/shift [round_up(c,V)]  (V as above: 4 for float32 ops, 8 for 16-bit ops)
     *   STEM:      wgt = [27][round_up(cout,4)] ; scale/shift [round_up(cout,4)]
     *   SE_FC:     wgt = W1[ldc][R4] (ABI 7: the Keras kernel [1,1,C,R] as it is, rows padded to R4 = round_up(reduced, 4)), b1 [R4],
 *              wgt2 = W2[reduced][ldc], b2 [ldc], ldc = round_up(c,4); all 16-byte aligned
     *   WSUM:      wgt = alpha[4]
     *   (the fused block ops document their packed layouts at their yr_op_kind above) */
    const float* wgt;    int64_t wgt_off;
    const float* scale;  int64_t scale_off;
    const float* shift;  int64_t shift_off;
    const float* wgt2;   int64_t wgt2_off;
    const float* b1;     int64_t b1_off;
    const float* b2;     int64_t b2_off;
    /* ---- ABI 7: the "SE tail" - squeeze-excite finished by the op that produces the map (csrc/se_tail.h).  An op that writes
     * per-workgroup channel sums to `gate` (DEPTHWISE SE form, MBX, STEMBLOCK without projection, HEAD) and has gate_out set also
     * runs the SE block's FC pair (efficientnet.py:419-434): the workgroup that completes an image's `se_reduced` rows adds them up
     * in index order, divides by h * w and writes sigmoid(W2 . swish(W1 . mean + b1) + b2) to gate_out[b] - what an SE_FC op with
     * k = h * w reading `gate` would have written (same values to float32 rounding), without the launch. */
    float* gate_out;  int32_t gate_out_buf;  int32_t gate_out_ld;   /* float32 [B][gate_out_ld], gate_out_ld >= round_up(cout, 4) */
    int32_t se_hidden;    /* hidden width R of the FC pair */
    int32_t reserved0;    /* a two-output POINTWISE op (YR_PWF_TWO_OUT): the second output's yr_act | YR_PW2_POOLED; else 0 */
    const float* se_w;  int64_t se_w_off;   /* W1 [ldc][R4] (Keras kernel [1,1,C,R], rows padded to R4 = round_up(R, 4)) | W2 [R][ldc] | b1 [R4] | b2 [ldc], ldc = round_up(cout, 4) */
    uint32_t* sync;       /* [batch] arrival counters: zero before the launch, zero again after it.  Plan ops: assigned by yr_forward
                             from the tail of the workspace (cleared at the start of every pass); yr_op_run: the caller's */
} yr_op;

/* Buffer table entry of a plan: per-image size in BYTES and either an arena
 * offset (per-image bytes, a multiple of 16; the runtime multiplies by batch) or an
 * external slot (0 = input images, 1..3 = y1..y3; always float32). */
typedef struct {
    int64_t bytes_per_image;
    int64_t arena_off_per_image;   /* -1 for external buffers */
    int32_t external_slot;         /* -1 for arena buffers */
    int32_t dtype;                 /* yr_dtype of the buffer's elements */
} yr_buf;

typedef struct yr_handle yr_handle;

const char* yr_last_error(void);
/* The name of the kernel instantiation the calling thread's last launch chose (spelled like the symbol, e.g. "dwp_kernel<bf16,3,0,1,4>";
 * what yr_forward_profile reports per launch), "" before any launch.  A static string: valid for the life of the library. */
const char* yr_last_kernel(void);
int yr_abi_version(void);
/* sizeof(yr_src) / sizeof(yr_op) / sizeof(yr_buf) / sizeof(yr_ingest_geom) / sizeof(yr_augment_geom) for which = 0 / 1 / 2 / 3 / 4 (else 0): lets a binding that restates the
 * structs (ctypes, cgo, JNA ...) verify its layout against the library's at load time. */
int yr_abi_sizeof(int which);

/* ---- whole-graph runtime: replaces tf.keras.Model.__call__ on the graph built by
 * yolov3_body (model.py:170-342; called at yolo.py:152, map.py:111). */
int yr_create(const yr_op* ops, int n_ops, const yr_buf* bufs, int n_bufs, yr_handle** out);
void yr_destroy(yr_handle* h);
/* ---- the same from ONE self-contained byte blob (yoloret_amd: Model.save_plan(); layout below): op list, buffer
 * table, parameter blob and the autotuned tile tables of a compiled model.  A host without the Python graph compiler
 * (C, C++, Go/cgo, JNI ...) instantiates "MobileNetV2x0.75 @416, bf16" from a file with this one call: the handle
 * comes back with its weights on the device and its tile tables installed.  Replaces yolov3_body + load_weights
 * (model.py:170-342, yolo.py:82-87) for deployments.  All fields little-endian:
 *   char magic[8] = "YRPLAN\0\0"; u32 abi (= YR_ABI_VERSION); u32 n_ops; u32 n_bufs; u32 sizeof(yr_op);
 *   u32 sizeof(yr_buf); u32 n_tables; u64 n_weight_floats; i32 in_h, in_w; i32 out_hwc[3][3] (y1, y2, y3: h, w, c);
 *   i32 reserved[3];   -- 96 bytes
 *   yr_op ops[n_ops] (pointer fields zero); yr_buf bufs[n_bufs]; float weights[n_weight_floats];
 *   n_tables x { i32 batch; i32 cfg[n_ops]; }   (yr_set_tuning tables) */
int yr_create_from_blob(const void* blob, size_t bytes, yr_handle** out);
/* Input / output geometry of a handle made by yr_create_from_blob (YR_ERR_STATE for other handles):
 * in_hw[2] = network input (h, w); out_hwc[9] = (h, w, c) of y1, y2, y3 (c = A*(C+5), dense). */
int yr_plan_io_dims(const yr_handle* h, int32_t* in_hw, int32_t* out_hwc);
/* Copies the flat fp32 parameter blob (host) to the device; owned by the handle.
 * Replaces tf.keras.Model.load_weights (yolo.py:87) once weights are in blob order. */
int yr_load_weights(yr_handle* h, const float* host_blob, size_t n_floats);
/* Bytes of caller-owned device workspace yr_forward needs for `batch` images (the arena of intermediate tensors followed by the
 * SE-tail arrival counters of the plan's ops, 4 * batch bytes each). */
size_t yr_workspace_bytes(const yr_handle* h, int batch);
/* images [B,H,W,3] -> y1,y2,y3 raw logits [B,G,G,A*(C+5)], G = H/32, H/16, H/8.
 * The pass (and yr_autotune, yr_forward_ranges, yr_forward_profile, which take the same buffers) writes only the B x G x G x A*(C+5)
 * floats of each output and the first yr_workspace_bytes(h, batch) bytes of `workspace`; no byte outside the B x H x W x 3 image
 * elements, and nothing the workspace held before the call, influences a logit; images, outputs and workspace need 16-byte
 * alignment and no more (inside the arena a buffer of image b starts at a multiple of 16 bytes - an odd batch gives its ops
 * pointers aligned to just that). */
int yr_forward(yr_handle* h, const float* images, int batch, float* y1, float* y2, float* y3,
               void* workspace, size_t workspace_bytes, void* stream);
/* Measurement aid: the same replay with a hipEvent pair around every op, `iters` times.
 * ms_per_op [n_ops] gets each op's average duration; kernel_names [n_ops] (nullable) gets a static
 * string naming the kernel symbol the op dispatched to.  Synchronises the stream. */
int yr_forward_profile(yr_handle* h, const float* images, int batch, float* y1, float* y2, float* y3,
                       void* workspace, size_t workspace_bytes, void* stream, int iters,
                       float* ms_per_op, const char** kernel_names);
/* The same pass, instrumented: max_abs_per_op[n_ops] (host) receives the largest |value| among the float32 k-space sources each op
 * reads (+inf where a NaN was seen; 0 for ops without such sources).  A float32 plan's SPLIT-form ops (POINTWISE without
 * YR_PWF_F32_MFMA, MBR / MBE with YR_MBR_SPLIT, HEAD) carry their operands as two float16 planes and need |x| < 65504 - the reference's float32
 * convolutions have no such bound (model.py:20-30; MobileNetV2's linear bottlenecks and residual sums are unclamped, override.py:290-341).
 * yoloret_amd's Model runs this once per set of weights on its first batch and rebuilds the plan with the ops beyond 60000 on the
 * float32-MFMA forms (Model.check_ranges); a host without it does the same through this call.  Synchronises the stream. */
int yr_forward_ranges(yr_handle* h, const float* images, int batch, float* y1, float* y2, float* y3,
                      void* workspace, size_t workspace_bytes, void* stream, float* max_abs_per_op);
/* Per-op tile autotuning for `batch` images: times every pointwise tile shape on every pointwise op (and a list of
 * output tiles on every MBH / MBX op) and remembers the fastest for later yr_forward calls with the same batch (numerics do not depend on the
 * shape).  Runs the forward once first; synchronises the stream. */
int yr_autotune(yr_handle* h, const float* images, int batch, float* y1, float* y2, float* y3,
                void* workspace, size_t workspace_bytes, void* stream, int iters);
/* The autotuned table for `batch`: one int per plan op - POINTWISE: 0 = heuristic, else the 1-based tile shape;
 * MBH, MBX: 0 = heuristic, else the output tile as th << YR_MBH_TH_SHIFT | tw << YR_MBH_TW_SHIFT; every other op kind: 0.  yr_get_tuning returns YR_ERR_STATE if that batch has not been tuned; yr_set_tuning installs a table
 * saved from an earlier run (tune once, deploy many: n must equal yr_plan_num_launches). */
int yr_get_tuning(const yr_handle* h, int batch, int32_t* cfg_per_op, int n);
int yr_set_tuning(yr_handle* h, int batch, const int32_t* cfg_per_op, int n);
/* Number of kernel launches one yr_forward enqueues. */
int yr_plan_num_launches(const yr_handle* h);

/* ---- single fused ops (device pointers inside `op`); parity-testable in isolation. */
int yr_op_run(const yr_op* op, int batch, void* stream);
/* How a YR_OP_HEAD launch cuts an h x w map into nsy x nsx regions (a function of the shape alone): the rows of the squeeze-excite
 * sums buffer such an op writes per image = nsy * nsx (its se_reduced). */
int yr_head_regions(int h, int w, int32_t* nsy, int32_t* nsx);
/* ... and of the WALKING form of YR_OP_HEAD (YR_HEAD_WALK): rows = strips of 14 columns x row segments (its se_reduced). */
int yr_head_walk_rows(int h, int w, int32_t* rows);
/* ... and of its WEIGHT-STREAMING form (YR_HEAD_STREAM): rows = strips x row segments x waves per workgroup. */
/* chunks of 32 channels the pixel-stationary POINTWISE form (YR_PWF_STATIONARY) runs a k space of kp channels with - what the plan
 * pads the weight planes to (1 .. 10, 12, 16); 0: the form does not take a k space this deep. */
int yr_pwt_chunks(int kp);
int yr_head_stream_rows(int h, int w, int32_t* rows);

/* ---- preprocessing (the step before the path): decoded uint8 [ih,iw,3] image (device) ->
 * letterboxed float32 [H,W,3] network input.  Replaces tf.io.decode_image(dtype=float32)'s /255
 * (yolo.py:106) + letterbox_image (utils.py:67-83: bilinear half-pixel resize, zero pad). */
int yr_letterbox(const unsigned char* src_u8, int ih, int iw, float* dst, int H, int W, void* stream);
/* The same for a batch of EQUALLY sized decoded images [B,ih,iw,3] -> [B,H,W,3] in one launch: the ingestion path of a
 * resident batch (uint8 over PCIe is a quarter of the float32 bytes; SURVEY.md 8(d) "incl. H2D"). */
int yr_letterbox_batch(const unsigned char* src_u8, int batch, int ih, int iw, float* dst, int H, int W, void* stream);

/* ---- decode: replaces yolo_head + yolo_correct_boxes + yolo_boxes_and_scores
 * (model.py:344-428) for the three scales at once, per image.
 *   y[s]      [B,G_s,G_s,A*(C+5)] raw logits, s = 0,1,2 for strides 32,16,8
 *   anchors   host, 9x(w,h) in the order of model_data/yolo_anchors.txt; scale s uses
 *             anchor_mask [[6,7,8],[3,4,5],[0,1,2]][s] (model.py:444)
 *   image_hw  device int32 [B,2] original image (h,w) per image
 *   boxes     [B,N,4] (ymin,xmin,ymax,xmax) fp32, N = A*sum(G_s^2)
 *   scores    [B,C,N] fp32, CLASS-MAJOR (score = conf*prob, model.py:426) */
int yr_decode(const float* y1, const float* y2, const float* y3, int batch, int in_h, int in_w,
              int num_anchors, int num_classes, int num_scales, const float* anchors_host,
              const int32_t* image_hw, float* boxes, float* scores, void* stream);
/* The same with the zoom-in test-time-augmentation pass of yolo_boxes_and_scores (model.py:408-417, enabled by
 * YoloModel.call(zoom_in=True), yolo.py:154-159): z[s] are the logits of the network run on the centre crop;
 * their box_xy / box_wh are mapped back as xy*zoom_mul + zoom_add, wh*zoom_mul (the reference hard-codes
 * 224/416 and (416-224)/(2*416)) and concatenated with the plain pass on the ANCHOR axis, so a cell holds 2A
 * boxes: boxes [B,2N,4], scores [B,C,2N], index ((h*G+w)*2A + pass*A + a) inside a scale. */
int yr_decode_zoom(const float* y1, const float* y2, const float* y3, const float* z1, const float* z2,
                   const float* z3, float zoom_mul, float zoom_add, int batch, int in_h, int in_w,
                   int num_anchors, int num_classes, int num_scales, const float* anchors_host,
                   const int32_t* image_hw, float* boxes, float* scores, void* stream);

/* yolo_head alone (model.py:344-371): one scale, reference layouts
 * box_xy/box_wh [B,G,G,A,2], conf [B,G,G,A,1], probs [B,G,G,A,C]; `scores` (nullable)
 * receives conf*probs [B,G,G,A,C] (model.py:426). */
int yr_yolo_head(const float* feats, int batch, int gh, int gw, int num_anchors, int num_classes,
                 const float* anchors_host /*A x (w,h)*/, int in_h, int in_w,
                 float* box_xy, float* box_wh, float* conf, float* probs, float* scores, void* stream);
/* yolo_correct_boxes (model.py:374-399): n = number of (xy,wh) pairs per image. */
int yr_correct_boxes(const float* box_xy, const float* box_wh, int batch, int64_t n_per_image,
                     int in_h, int in_w, const int32_t* image_hw, float* boxes, void* stream);

/* ---- per-(image,class) hard NMS: replaces the loop of tf.image.non_max_suppression
 * calls at model.py:474-480 (NonMaxSuppressionV3 semantics).
 *   out_idx [B,C,max_boxes] int32 box indices in pick order (unused tail = -1)
 *   out_count [B,C] int32 */
int yr_nms(const float* boxes, const float* scores, int batch, int n, int num_classes, int max_boxes,
           float score_thr, float iou_thr, int32_t* out_idx, int32_t* out_count, void* stream);

/* ---- gather + cast: model.py:481-490.  Fixed-size padded records so that the
 * multi-GPU all-gather moves one dense tensor:
 *   det [B, C*max_boxes, 6] int32 words = {ymin,xmin,ymax,xmax (int32, truncated),
 *        score (fp32 bits), class (int32)}, rows ordered class-ascending then pick
 *        order, compacted to the front; det_count [B] int32. */
int yr_pack_detections(const float* boxes, const float* scores, const int32_t* nms_idx,
                       const int32_t* nms_count, int batch, int n, int num_classes, int max_boxes,
                       int32_t* det, int32_t* det_count, void* stream);

/* ---- YoloLoss.call, GIOU branch (model.py:607-671, with yolo_head(calc_loss=True) :344-369 and do_giou_calculate,
 * utils.py:9-53) for ONE scale, forward only; added under ABI 9 (additive: no struct or existing entry changed).
 *   feats     [B,gh,gw,A,5+C] raw logits, dense float32;  y_true: same shape, the rows preprocess_true_boxes
 *             (utils.py:298-376) writes: (x, y, w, h) relative to the input, object flag, class bits
 *   anchors   host, the A x (w,h) anchors of THIS scale (model.py:605);  in_h, in_w = grid * grid_step (:628)
 *   out5      device float32 {loss, giou_loss, confidence_loss, class_loss, ignore_sum}: the three sums divided by B
 *             (:662-668), their total, and sum(ignore_mask) over every cell (:671)
 * As in the reference, the labelled boxes are gathered over the WHOLE batch (:643): a prediction of one image is
 * compared with the labelled boxes of every image of the call; with no labelled box at all every cell is ignored.
 * Per-element arithmetic is float32 in the reference's order; the sums are float64 in a fixed order, rounded once:
 * the same call gives the same bits.  Non-finite logits are outside the contract.  Three launches on `stream`, no
 * host synchronisation.  `workspace`: device memory, 16-byte aligned, at least the number of bytes the first
 * entry returns (0 for bad sizes); its contents before the call do not matter. */
size_t yr_yolo_loss_workspace_bytes(int batch, int gh, int gw, int num_anchors);
int yr_yolo_loss(const float* feats, const float* y_true, int batch, int gh, int gw, int num_anchors,
                 int num_classes, const float* anchors_host /*A x (w,h)*/, int in_h, int in_w,
                 float ignore_thresh, void* workspace, size_t workspace_bytes,
                 float* out5 /*device*/, void* stream);

/* ---- the gradient of that loss with respect to its logits: what differentiating the scalar of YoloLoss.call (model.py:607-671,
 * GIOU branch; through yolo_head(calc_loss=True) :344-369 and do_giou_calculate, utils.py:9-53) gives at `feats`, as _train_step
 * does (code/yolo3/train.py:18-46); added under ABI 9 (additive: no struct or existing entry changed).  Arguments, workspace
 * (yr_yolo_loss_workspace_bytes) and checks as yr_yolo_loss, and out5 receives exactly the bits yr_yolo_loss writes, in the same
 * three launches.
 *   upstream_dev  device, one float32: the cotangent of the scalar loss, read by the kernel; null stands for 1.  It multiplies each
 *                 finished float32 element as the last operation (a power of two scales the result exactly)
 *   dfeats        device float32 [B,gh,gw,A,5+C] = upstream * d loss / d feats with m = B.  EVERY element is written, zeros
 *                 included: nothing needs zeroing first.  4-byte alignment suffices
 * Rules (TensorFlow's autodiff; unpinned by the reference like the forward, see csrc/loss.hip): ignore_mask is a constant and
 * best_iou contributes nothing; channel 4: (om + (1 - om) * ignore) * (sigmoid(x4) - om) / m; channels 5..: om * (sigmoid(x_c) -
 * t_c) / m; channels 0-3: -om / m * d giou / d(pred box) chained through the corners and the decode, the true box a constant;
 * Maximum / Minimum send the gradient to their first operand on a tie (the prediction; maximum(zero, v) passes it only where
 * v > 0), divide_no_nan passes none where the denominator is 0.  Box and class channels are exactly 0 where the object flag is 0.
 * Float32 arithmetic; no atomics beyond the forward's list counter: the same call gives the same bytes.  This is the gradient at
 * the logits only: no backward through the network. */
int yr_yolo_loss_grad(const float* feats, const float* y_true, int batch, int gh, int gw, int num_anchors,
                      int num_classes, const float* anchors_host /*A x (w,h)*/, int in_h, int in_w,
                      float ignore_thresh, void* workspace, size_t workspace_bytes,
                      const float* upstream_dev /*device, may be null = 1*/, float* out5 /*device*/,
                      float* dfeats /*device*/, void* stream);

/* ---- VOC matching of detections to ground truth: the greedy loop of MAPCallback.calculate_aps (code/yolo3/map.py:157-215)
 * on the device, per image; added under ABI 9 (additive: no struct or existing entry changed).
 *   det [B,rows,6], det_count [B]   exactly what yr_pack_detections writes; only the first det_count[b] rows of image b
 *                                   are read, in any order (rows of a class need not be contiguous or sorted)
 *   gt [B,max_gt,5] float32         (xmin, ymin, xmax, ymax, label): the label file's order; the first gt_count[b] [B]
 *                                   rows of image b are read.  max_gt may be 0, gt then null
 *   flags [B,rows] int32            1 true positive, 0 false positive; -1 for rows at or beyond det_count[b] and for rows
 *                                   whose class is outside [0, num_classes)
 *   npos [B,num_classes] int32      valid ground-truth rows of image b with label == class (labels outside the range or
 *                                   with a fractional part count nowhere)
 * Rule, per (image, class): detections in score order (float32 values, descending; ties by lower row index); the best box
 * is the ground-truth row of that class with the largest IoU (VOC +1 convention, float64, ties to the lowest index), chosen
 * before the claim check; true positive iff IoU > iou_thr (strict) and the box is unclaimed, which claims it.  Since a
 * detection only competes inside its image and class, these are the verdicts of the reference's pass over the data set.
 * Scores and coordinates must be finite, and max >= min on both axes of every box.  One launch on `stream`, no workspace,
 * no host synchronisation; the same call gives the same bytes. */
#define YR_VOC_MAX_ROWS 4096   /* rows per image (C * max_boxes; the reference's largest is 80 * 20) */
#define YR_VOC_MAX_GT   512    /* padded ground-truth rows per image */
int yr_voc_match(const int32_t* det, const int32_t* det_count, int batch, int rows, int num_classes,
                 const float* gt, const int32_t* gt_count, int max_gt, double iou_thr,
                 int32_t* flags, int32_t* npos, void* stream);

/* ---- preprocess_true_boxes (code/yolo3/utils.py:298-376) for a whole batch on the device: ground-truth boxes -> the y_true
 * tensors yr_yolo_loss reads; added under ABI 9 (additive: no struct or existing entry changed).
 *   true_boxes [B,max_boxes,5] float32 rows (x_min, y_min, x_max, y_max, class) in pixels of the network input, padded with
 *                                   zero rows: the host function's argument for one image, stacked over the batch
 *   anchors    host, 9 x (w,h) float32: ALL anchors (:339), not those of one scale
 *   y1..y3     output l < num_scales is dense float32 [B, in_h / s, in_w / s, 3, 5+C] with s = (32, 16, 8)[l] and the anchors
 *              ([6,7,8], [3,4,5], [0,1,2])[3 - num_scales + l] (:317-318: with fewer than 3 scales the SMALL anchors meet
 *              stride 32, as in the reference); the others are not touched and may be null.  Every element is written:
 *              nothing needs zeroing first
 *   skipped    [B] int32, may be null: rows of image b that were not written, see below
 * Contract: the bytes equal the host function's, image by image, for every input on which it neither raises nor writes outside
 * its grids.  That fixes the arithmetic: centre = floor((min + max) / 2) and size = max - min in float32 (:321-322); the four
 * relative values are float64 quotients rounded once to float32 (:323-324); a row is valid when its float32 width is > 0 (:342);
 * the best anchor is the first maximum over the nine anchors of the float32 IoU of the two centred boxes in the operation order of
 * do_giou_calculate(anchor_box, bbox, mode='iou') with divide_no_nan (:349-354; parity is claimed for float32 anchors); the r-th
 * VALID row supplies the anchor while row r of the UNFILTERED rows supplies the coordinates, the class and the cell (:356-368);
 * the cell is floor(relative centre * grid) with the product in float64 (:359-362); entry[0:4] = the relative values,
 * entry[4] = 1, entry[5 + int(class)] = 1 with int() truncating toward zero (:364-368); the last row in index order that lands
 * on a (scale, cell, slot) leaves its box there and the class bits of all of them accumulate.
 * Rows the host function does not write safely (it raises, or a negative index wraps) write nothing and are counted in
 * skipped[b]: a row with a non-finite value among its five is removed before anything else, so that the remaining rows are
 * encoded exactly as if it had not been in the list; a row whose truncated class is outside [0, C) or whose cell is outside the
 * grid is dropped when its turn to be written comes.  (A row that is never a supplier of coordinates - beyond the number of
 * valid rows, or paired with an anchor of a scale that num_scales leaves out - is not looked at and not counted.)
 * Two launches on `stream` (zero-fill, then one workgroup per image), no workspace, no host synchronisation, no atomics: the
 * same call gives the same bytes.  Outputs need 4-byte alignment only. */
#define YR_ENC_MAX_BOXES 256   /* rows per image (one lane each) */
int yr_encode_labels(const float* true_boxes /*device [B,T,5]*/, int batch, int max_boxes /*T*/,
                     int in_h, int in_w, const float* anchors_host /*9 x (w,h)*/,
                     int num_classes, int num_scales,
                     float* y1, float* y2, float* y3 /*device; only the first num_scales are used, the others may be null*/,
                     int32_t* skipped /*device [B], may be null*/, void* stream);

/* ---- ragged batched ingest: B decoded uint8 images of different sizes -> the float32 [B,H,W,3] network input in one launch,
 * and - for the validation data path - their ground-truth boxes mapped into that input in the same launch; added under ABI 9
 * (additive: no struct or existing entry changed; yr_abi_sizeof(3) reports sizeof(yr_ingest_geom)).  Replaces, after the host's
 * image decode and text parse, per image:
 *   YR_INGEST_LETTERBOX  letterbox_image (code/yolo3/utils.py:67-83) behind code/yolo.py:105-112: the geometry and the bytes of
 *                        yr_letterbox, for every consumer of mixed-size images (one copy and one launch instead of B of each);
 *   YR_INGEST_VALIDATE   get_random_data(train=False, zoom_in=False) (code/yolo3/utils.py:239-295) as Dataset.parse_text calls it
 *                        (code/yolo3/data.py:71-121).  This is NOT letterbox_image's arithmetic: the geometry is float32, the
 *                        pad offset is int((h - nh) / 2) with the UNTRUNCATED nh, and the boxes are mapped with the untruncated
 *                        nw, nh, dx, dy.  At 96x96 a 5x7 image sits at dy = 13 here and at dy = 14 there. */
#define YR_INGEST_LETTERBOX 0   /* utils.py:67-83 - exactly the geometry yr_letterbox computes */
#define YR_INGEST_VALIDATE  1   /* utils.py:239-252, get_random_data(train=False, zoom_in=False) */
#define YR_INGEST_MAX_BOXES 256 /* input rows per image (one lane each) */
typedef struct {                /* 64 bytes; yr_abi_sizeof(3) reports it */
    int64_t src_off;            /* byte offset of image b in the packed source, a multiple of 16 */
    int32_t ih, iw, nh, nw, dy, dx;   /* source size; size and offset of the resized window inside H x W */
    float   nh_f, nw_f, dy_f, dx_f;   /* VALIDATE: the untruncated float32 values the boxes use; LETTERBOX: 0 */
    int32_t reserved[4];        /* 0 */
} yr_ingest_geom;
/* The one place where the arithmetic of both rules lives (utils.py:76-79 | :152-155,239-242,247-250); pure host, no device touched.
 *   dims_host [B][2] = (ih, iw) per image;  geom_host [B] receives the table;  packed_bytes (nullable) the size of the packed
 *   source: the images [ih][iw][3] uint8 back to back, each offset rounded up to 16, the end rounded up to 16 as well
 * LETTERBOX: the ratio min(W / iw, H / ih) in float64, nh / nw truncated, dy = (H - nh) / 2 and dx = (W - nw) / 2 floor-divided.
 * VALIDATE: float32 in TF's order - m = min(w / iw, h / ih); nh_f = ih * m; nw_f = iw * m; dx_f = (w - nw_f) / 2;
 * dy_f = (h - nh_f) / 2; the integer fields are the truncations of those four.
 * YR_ERR_ARG, with the image's index in the message, where nh or nw truncates to 0 (tf.image.resize raises there too).
 * A caller places the table next to the images in its staging buffer and uploads both with one copy. */
int yr_ingest_geometry(int mode, int batch, const int32_t* dims_host /*[B][2] = ih, iw*/, int H, int W,
                       yr_ingest_geom* geom_host /*[B]*/, int64_t* packed_bytes);
/* The launch.  `mode` is the rule the table was computed with (the table lives on the device; the entry does not read it).
 * Image part (utils.py:81-82 | :246-252,277) - every element of dst is written: inside the nh x nw window of image b at (dy, dx)
 * u8 * (1/255), then the bilinear half-pixel resize in yr_letterbox's operation order with the scales (float)ih / (float)nh and
 * (float)iw / (float)nw, then in VALIDATE mode clip_by_value(0, 1); zeros outside.  In LETTERBOX mode the bytes equal
 * yr_letterbox's image by image.
 * Box part (VALIDATE mode only; boxes_in non-null in LETTERBOX mode is YR_ERR_ARG; boxes_in null: images only, boxes_out and
 * kept are not touched), all float32:
 *   boxes_in [B,max_in,5]   rows (xmin, ymin, xmax, ymax, label) in pixels of the SOURCE image - the label file's order, what
 *                           yr_voc_match reads; the first box_count[b] [B] rows of image b are read (clamped to 0..max_in);
 *                           max_in <= YR_INGEST_MAX_BOXES
 *   x' = x * nw_f / iw + dx_f, y' = y * nh_f / ih + dy_f, left to right (:253-256); each coordinate clipped to [0, W - 1] /
 *   [0, H - 1] (:258-273); a row is kept iff xmax' - xmin' > 1 and ymax' - ymin' > 1, both strict (:289-291); the first
 *   max_boxes kept rows, in input order (:292-293), go to the front of boxes_out[b] [B,max_boxes,5] as (xmin', ymin', xmax',
 *   ymax', label) - yr_encode_labels's input -, the rest of boxes_out[b] is zero; kept[b] [B] (nullable) is their number.  The
 *   label's bits are copied through.  Coordinates must be finite.
 * One launch on `stream` (the box part is one extra workgroup per image of the same grid), no workspace, no atomics, no host
 * synchronisation; the same call gives the same bytes.  src_u8, geom and dst need 16-byte alignment, B * H * W < 2^31. */
int yr_ingest_batch(int mode, const unsigned char* src_u8 /*device, packed*/, const yr_ingest_geom* geom /*device [B]*/, int batch,
                    float* dst /*[B,H,W,3]*/, int H, int W,
                    const float* boxes_in /*[B,max_in,5] or null*/, const int32_t* box_count /*[B]*/, int max_in,
                    float* boxes_out /*[B,max_boxes,5]*/, int32_t* kept /*[B], may be null*/, int max_boxes, void* stream);

/* ---- training data transform: get_random_data(train=True) (code/yolo3/utils.py:170-237, then :258-293) for a ragged batch of
 * decoded uint8 images -> the float32 [B,H,W,3] network input and the mapped boxes; added under ABI 9 (additive: no struct or
 * existing entry changed; yr_abi_sizeof(4) reports sizeof(yr_augment_geom)).  Per image, in the reference's order: random
 * aspect and scale, resize (bilinear, half-pixel centres, no antialias), crop and / or pad to H x W, flip, random_hue,
 * random_saturation, adjust_gamma, random_contrast, clip_by_value(0, 1); the boxes follow the geometry and the flip.
 * random_jpeg_quality (:228-230, ON by default in the reference) is a stage of its own behind these launches: yr_jpeg_roundtrip_batch
 * below.  NOT built: random_brightness (val), noise, blur, zoom_in (all off by default).
 * TensorFlow is not available to this project: adjust_hue and adjust_saturation follow TF 2.x's fused CPU kernels as restated
 * from memory in tests/augment_ref.py, which is the definition the kernels are tested against. */
#define YR_AUG_HUE      1       /* stage mask: random_hue        (the reference's `hue > 0`) */
#define YR_AUG_SAT      2       /*             random_saturation (`sat > 0`) */
#define YR_AUG_GAMMA    4       /*             adjust_gamma      (`min_gamma < max_gamma`) */
#define YR_AUG_CONTRAST 8       /*             random_contrast   (`cont > 0`) */
#define YR_AUG_NOFLIP   16      /*             set: `flip=False`, the flip draw is ignored */
#define YR_AUG_ALL      31
typedef struct {                /* 96 bytes; yr_abi_sizeof(4) reports it */
    int64_t src_off;            /* byte offset of image b in the packed source, a multiple of 16 (yr_ingest_geometry's packing) */
    int32_t ih, iw;             /* source size */
    int32_t rh, rw;             /* the size the source is resized to: int(nh), int(nw) */
    int32_t cy, cx;             /* crop offset inside the resized image */
    int32_t wh, ww;             /* the visible window: min(H, rh) x min(W, rw) after a crop, rh x rw without */
    int32_t py, px;             /* where the window sits in the H x W canvas (before the flip) */
    int32_t flip;               /* 1: the canvas is mirrored, out[y][x] = canvas[y][W - 1 - x] */
    int32_t clamped;            /* 1: max(ratio, 1) took the 1 (information only) */
    int32_t reserved[2];        /* 0 */
    float   nh_f, nw_f, dy_f, dx_f;   /* the untruncated float32 values the boxes use */
    float   hue6, sat, gamma, cont;   /* delta * 6, saturation factor, gamma, contrast factor; the identity (0, 1, 1, 1) for a stage that is off */
} yr_augment_geom;
/* The one place where the arithmetic of utils.py:171-181 and of the ten draws lives; pure host, no device touched, all float32,
 * uniform(lo, hi) = lo + u * (hi - lo) with the bounds rounded to float32 once from the double expression (1 - jitter, ...):
 *   draws_host [B][10] = j1, j2, scale, dx, dy, flip, hue, sat, gamma, contrast, each u in [0, 1)
 *   new_ar = (W / H) * (U(j1; 1 - jitter, 1 + jitter) / U(j2; same));  scale = U(min_scale, max_scale)
 *   ratio = max(new_ar < 1 ? scale * new_ar : scale / new_ar, 1)
 *   (nw, nh) = new_ar < 1 ? (ratio * H, scale * H) : (scale * W, ratio * W);  dx = U(0, W - nw);  dy = U(0, H - nh)
 *   nw > W or nh > H: crop at (int(max(-dy, 0)), int(max(-dx, 0))) to min(H, int(nh)) x min(W, int(nw)); always: pad at
 *   (int(max(dy, 0)), int(max(dx, 0)));  flip iff the flip draw < 0.5 and YR_AUG_NOFLIP is clear
 *   hue6 = U(-hue, hue) * 6;  sat = U(1 - sat, 1 + sat);  gamma = U(min_gamma, max_gamma);  cont = U(1 - cont, 1 + cont)
 * dims_host and packed_bytes as in yr_ingest_geometry.  YR_ERR_ARG, with the image's index in the message, where a resized side
 * truncates to 0 or where a precondition of crop_to_bounding_box / pad_to_bounding_box fails (TensorFlow raises there too; no
 * draw in [0, 1) is known to get there), and for parameters outside jitter in [0, 1), hue in [0, .5], sat and cont in [0, 1]. */
int yr_augment_geometry(int batch, const int32_t* dims_host /*[B][2] = ih, iw*/, int H, int W, const float* draws_host /*[B][10]*/,
                        int stages, double jitter /*.3*/, double min_scale /*.25*/, double max_scale /*2*/, double hue /*.5*/,
                        double sat /*.5*/, double min_gamma /*.8*/, double max_gamma /*2*/, double cont /*.1*/,
                        yr_augment_geom* geom_host /*[B]*/, int64_t* packed_bytes);
/* Bytes of the workspace of the launch below: one slot of three float32 channel sums per image workgroup. */
size_t yr_augment_workspace_bytes(int batch, int H, int W);
/* The launches.  `stages` is the mask the table was computed with.  Every element of dst [B,H,W,3] is written; with boxes_in
 * (the arguments and the rules of yr_ingest_batch's box part, plus (xmin, xmax) -> (W - xmax, W - xmin) on a flipped image) every
 * element of boxes_out and kept; boxes_in null: images only.  Contrast uses the mean of each channel over the whole H x W canvas,
 * padding included, after gamma: launch 1 stores every pixel through gamma and one slot of channel sums per workgroup, launch 2
 * adds an image's slots in a fixed order, applies contrast and the clip in place and maps the boxes in one extra workgroup per
 * image.  Without YR_AUG_CONTRAST launch 1 clips, launch 2 carries only the boxes and the workspace may be null.  No atomics; the
 * same call gives the same bytes.  H * W must be a multiple of 4; src_u8, geom, dst and workspace need 16-byte alignment;
 * B * H * W < 2^31.  Pixel values before gamma are non-negative by construction, so pow sees no negative base. */
int yr_augment_batch(const unsigned char* src_u8 /*device, packed*/, const yr_augment_geom* geom /*device [B]*/, int batch, int stages,
                     float* dst /*[B,H,W,3]*/, int H, int W,
                     const float* boxes_in /*[B,max_in,5] or null*/, const int32_t* box_count /*[B]*/, int max_in,
                     float* boxes_out /*[B,max_boxes,5]*/, int32_t* kept /*[B], may be null*/, int max_boxes,
                     void* workspace /*device*/, size_t workspace_bytes, void* stream);

/* ---- tf.image.random_jpeg_quality (code/yolo3/utils.py:228-230: convert_image_dtype to uint8, adjust_jpeg_quality, back to float32),
 * the last image step of get_random_data(train=True), for a batch of float32 canvases IN PLACE, one quality per image; added under
 * ABI 9 (additive: no struct or existing entry changed).  Entropy coding is lossless, so the encode and decode are integer arithmetic
 * without a bitstream: float -> uint8 (trunc(min(max(x * 255.5f, 0), 255))), RGB -> YCbCr, 2x2 chroma mean, forward DCT (jfdctint.c),
 * quantise with the Annex K tables scaled to the quality | dequantise, inverse DCT (jidctint.c), triangle-filter chroma upsampling,
 * YCbCr -> RGB, uint8 -> float (u * (1 / 255)f): 4:2:0, the "islow" DCT and fancy upsampling, libjpeg's and TensorFlow's defaults.
 * tests/jpeg_ref.py restates every step and is pinned byte for byte against Pillow on libjpeg-turbo; the kernels equal it bit for bit.
 * H and W must be multiples of 16 (whole MCUs; the network input is a multiple of 32): libjpeg's edge replication and dummy blocks
 * are not built.  The quality is drawn by the caller (TensorFlow: an int32 uniform over [min_jpeg_quality, max_jpeg_quality)). */
/* Bytes of the workspace of the launches below: the decoded Y plane and the two quarter-size chroma planes, uint8. */
size_t yr_jpeg_workspace_bytes(int batch, int H, int W);
/* Two launches: launch 1 reads the images and writes the decoded planes of every MCU to the workspace, launch 2 upsamples the
 * chroma, converts and overwrites every element of images.  quality [B] is read on the device and clamped there to 1..100 (libjpeg
 * reads 0 as 1).  No atomics, no host synchronisation; the same call gives the same bytes whatever the workspace held.  YR_ERR_ARG,
 * nothing written: H or W not a multiple of 16, a null pointer, B * H * W >= 2^31, batch > 65535, a workspace smaller than
 * yr_jpeg_workspace_bytes, images or workspace not 16-byte aligned. */
int yr_jpeg_roundtrip_batch(float* images /*device [B,H,W,3], in place*/, const int32_t* quality /*device [B]*/, int batch, int H, int W,
                            void* workspace /*device*/, size_t workspace_bytes, void* stream);

/* ---- training the output convolutions (the three *_y 1x1 convs, code/yolo3/model.py:111): what _train_step (code/yolo3/train.py:18-46)
 * does for them between the features and optimizer.apply_gradients when the body is frozen (code/train.py:150-171, "Train with frozen
 * layers first"); added under ABI 9 (additive: no struct or existing entry changed).  csrc/headtrain.hip has the kernels' forms.
 * Rows are float32, row-major over pixels, P = B * H * W: x [P][x_ld] with cin channels taken, dy / y [P][ld] with cout taken.
 * Weights are Wt[cout][kp], kp = round_up(cin, 4): the layout of YR_OP_POINTWISE, pad columns 0.  Every pointer needs 4-byte
 * alignment only (a dense row of 75 floats).  Operands and accumulation are float32 on the float32 matrix pipe.  1 <= cin, cout
 * <= 256, 1 <= pixels < 2^40, ld >= the channels taken; YR_ERR_ARG, nothing written, otherwise (also: a null pointer, byte offsets
 * beyond 2^63, a workspace that is short or not 16-byte aligned). */
/* the layer's forward (model.py:111, a bias-free 1x1 Conv2D): y[p][co] = sum_k x[p][k] * wt[co][k].  Every y[p][0..cout) is written
 * and nothing else; pad columns of wt are not read.  One launch. */
int yr_linear_forward(const float* x, int x_ld, const float* wt /*[cout][kp]*/, long long pixels, int cin, int cout,
                      float* y, int y_ld, void* stream);
/* d loss / d Wt, what tape.gradient (yolo3/train.py:39) gives for the layer's kernel: dwt[co][ci] = sum_p dy[p][co] * x[p][ci].
 * Two launches, no float atomics: stage 1 gives every workgroup a contiguous range of yr_linear_wgrad_chunk(pixels, cin, cout)
 * pixels - a function of its three arguments only, never of the device - and writes one partial [cout][kp] slab per range to the
 * workspace; stage 2 adds the slabs in index order and writes EVERY element of dwt, pad columns as +0.  Nothing needs zeroing
 * first, the workspace contents before the call do not matter, and the same call gives the same bytes.  Pad columns of the rows
 * (elements at and beyond cin / cout) are never read.  The two size entries return 0 for sizes the call refuses. */
int    yr_linear_wgrad_chunk(long long pixels, int cin, int cout);
size_t yr_linear_wgrad_workspace_bytes(long long pixels, int cin, int cout);
int    yr_linear_wgrad(const float* x, int x_ld, const float* dy, int dy_ld, long long pixels, int cin, int cout,
                       void* workspace /*device*/, size_t workspace_bytes, float* dwt /*[cout][kp]*/, void* stream);
/* Keras Adam's dense update (code/train.py:158 Adam(lr[0], epsilon=1e-8) behind optimizer.apply_gradients, yolo3/train.py:40), in place, one
 * launch for n elements, float32 operations in this order with nothing contracted:
 *   m = beta1 * m + (1 - beta1) * g;   v = beta2 * v + (1 - beta2) * (g * g);   w = w - alpha * m / (sqrt(v) + eps)
 * 1 - beta1 and 1 - beta2 are formed once in float32; alpha = float32(lr * sqrt(1 - beta2^t) / (1 - beta1^t)) is the caller's, from
 * float64.  TF 2.x OptimizerV2 Adam without amsgrad, restated (no TensorFlow where this is tested: tests/headtrain_ref.py is the
 * definition).  g is only read.  1 <= n <= 2^39. */
int yr_adam_step(float* w, float* m, float* v, const float* g, long long n,
                 float alpha, float beta1, float beta2, float eps, void* stream);

/* ---- backward operators of the layers behind the output convolutions (code/train.py:150-171 trains the neck and the heads: bias-free
 * 1x1 convolutions, k x k depthwise convolutions, BatchNorm, ReLU6 / Swish); added under ABI 9 (additive).  csrc/convgrad.hip has the
 * kernels' forms, tests/convgrad_ref.py is the definition (the reference's backward is TensorFlow's tape).  The conventions of the
 * entries above hold: float32, rows row-major over pixels with a leading dimension in floats, 4-byte alignment, no float atomics,
 * nothing read before the call wrote it, every named output element written and nothing else, the same call gives the same bytes.
 * YR_ERR_ARG, nothing written, for sizes outside the contract, a null pointer, a short or misaligned workspace. */
/* d loss / d x of yr_linear_forward: dx[p][ci] = sum_co dy[p][co] * wt[co][ci] on the float32 matrix pipe.  1 <= cin, cout <= 256,
 * 1 <= pixels < 2^40.  Every dx[p][0..cin) is written, dx[p][cin..dx_ld) is not touched; pad columns of wt and of dy are not read.
 * One launch. */
int yr_linear_dgrad(const float* dy, int dy_ld, const float* wt /*[cout][kp]*/, long long pixels, int cin, int cout,
                    float* dx, int dx_ld, void* stream);
/* Depthwise convolution on plain maps [B][H][W][ld] (C <= ld channels taken), taps w[k * k][C] (the Keras kernel [k,k,C,1] reshaped),
 * k in {3, 5}, stride in {1, 2}.  The padding is explicit: pad_top, pad_left in 0..k-1 and the output size (OH, OW), which must be
 * floor((H + pad_top + pad_bottom - k) / stride) + 1 for some pad_bottom in 0..k-1 (columns alike).  Taps are taken in the order
 * t = ty * k + tx, one fmaf each from +0; out-of-range taps contribute nothing.
 *   forward  y[b][oy][ox][c] = sum_t x[b][oy s - pad_top + ty][ox s - pad_left + tx][c] * w[t][c].  One launch.
 *   dgrad    dx[b][iy][ix][c] = sum over the taps with iy + pad_top - ty = oy s, ix + pad_left - tx = ox s inside the output of
 *            dy[b][oy][ox][c] * w[t][c]: a gather, every dx element written once.  One launch.
 *   wgrad    dw[t][c] = sum_{b,oy,ox} dy[b][oy][ox][c] * x[b][oy s - pad_top + ty][ox s - pad_left + tx][c].  Two launches: stage 1
 *            writes one partial [k * k][C] slab per yr_depthwise_wgrad_chunk(B, OH, OW, C, k) rows of the B * OH output rows - a
 *            function of its arguments only -, stage 2 adds the slabs in index order and writes every dw element.  The workspace
 *            (16-byte aligned) holds the slabs; its contents before the call do not matter.  The two size entries return 0 for
 *            sizes the call refuses. */
int    yr_depthwise_forward(const float* x, int x_ld, const float* w /*[k*k][C]*/, int B, int H, int W, int C, int k, int stride,
                            int pad_top, int pad_left, int OH, int OW, float* y, int y_ld, void* stream);
int    yr_depthwise_dgrad(const float* dy, int dy_ld, const float* w /*[k*k][C]*/, int B, int H, int W, int C, int k, int stride,
                          int pad_top, int pad_left, int OH, int OW, float* dx, int dx_ld, void* stream);
int    yr_depthwise_wgrad_chunk(int B, int OH, int OW, int C, int k);
size_t yr_depthwise_wgrad_workspace_bytes(int B, int OH, int OW, int C, int k);
int    yr_depthwise_wgrad(const float* x, int x_ld, const float* dy, int dy_ld, int B, int H, int W, int C, int k, int stride,
                          int pad_top, int pad_left, int OH, int OW, void* workspace /*device*/, size_t workspace_bytes,
                          float* dw /*[k*k][C]*/, void* stream);
/* Frozen BatchNorm (inference mode: per-channel scale and shift) + activation (act: YR_ACT_NONE, YR_ACT_RELU6 or YR_ACT_SWISH) on
 * rows [pixels][ld].  forward: u = z * scale[c] + shift[c] (a float32 multiply, then a float32 add), a = act(u); u (may be null) also
 * receives u, for the backward.  backward: dz = (da * act'(u)) * scale[c]; ReLU6: act' = 1 where 0 < u < 6, both strict
 * (TensorFlow's Relu6Grad), dz = +0 elsewhere; Swish: act' = sg (1 + u (1 - sg)), sg the forward kernels' sigmoid; none: u is not
 * read and may be null.  No gradient for scale or shift.  One launch each. */
int yr_bn_act_forward(const float* z, int z_ld, const float* scale, const float* shift, long long pixels, int C, int act,
                      float* a, int a_ld, float* u /*or null*/, int u_ld, void* stream);
int yr_bn_act_backward(const float* da, int da_ld, const float* u /*null for YR_ACT_NONE*/, int u_ld, const float* scale,
                       long long pixels, int C, int act, float* dz, int dz_ld, void* stream);

/* ---- BatchNorm (+ activation) in training mode (yolo3/model.py:24-105 puts a BatchNormalization, momentum 0.9, epsilon 1e-3, behind
 * every convolution of the neck and the heads, and the training step calls the model with training=True); added under ABI 9 (additive).
 * csrc/bntrain.hip has the kernels' forms, tests/bntrain_ref.py is the definition.  The conventions of the entries above hold: float32,
 * rows [pixels][ld] with C <= ld channels taken (pad columns neither read nor written), 4-byte alignment, no float atomics, nothing read
 * before the call wrote it, every named output element written and nothing else, the same call gives the same bytes.
 * 1 <= pixels < 2^40, 1 <= C < 2^31 - 64, eps >= 0 and finite, 0 <= momentum <= 1, act one of YR_ACT_NONE, YR_ACT_RELU6, YR_ACT_SWISH; the
 * workspace (device, 16-byte aligned, yr_bn_train_workspace_bytes(pixels, C) bytes: enough for either call) may hold anything before the
 * call.  YR_ERR_ARG, nothing written, for anything else, a null pointer, a short or misaligned workspace, one moving pointer without the
 * other.  Every operation is one IEEE float32 operation in this order, nothing contracted (N = pixels):
 *   forward   mean[c] = (sum_p z[p][c]) / (float)N;  var[c] = (sum_p (z[p][c] - mean[c])^2) / (float)N - the squared deviations about the
 *             finished mean, never E[z^2] - E[z]^2;  invstd[c] = 1.0f / sqrtf(var[c] + eps), both correctly rounded;
 *             xhat = (z - mean[c]) * invstd[c];  u = xhat * gamma[c] + beta[c] (a multiply, then an add);  a = act(u) (the forward
 *             kernels' activations).  The moving statistics, when given (both or neither), are updated in place as Keras' fused path
 *             does, which stores the UNBIASED variance of the batch: d = 1.0f - momentum;  moving_mean -= (moving_mean - mean) * d;
 *             moving_var -= (moving_var - var * bessel) * d,  bessel = (float)((double)N / (double)max(N - 1, 1)).  3 launches.
 *   backward  u and xhat are recomputed from z, mean, invstd, gamma and beta by the forward's operations (the same bits); g = da * act'(u)
 *             with the rules of yr_bn_act_backward (ReLU6: g = da where 0 < u < 6, both strict, +0 elsewhere; Swish: sg (1 + u (1 - sg)));
 *             dbeta[c] = sum_p g;  dgamma[c] = sum_p (g * xhat) (a product, then the sum);
 *             dz = ((g - dbeta[c] / (float)N) - xhat * (dgamma[c] / (float)N)) * (gamma[c] * invstd[c]).  dz may be null: it is not
 *             computed, dgamma and dbeta are the same bits.  2 launches either way.
 * Every per-channel sum has two stages: stage 1 gives each workgroup a contiguous range of yr_bn_train_chunk(pixels, C) pixels - a
 * function of its arguments only - and writes one [C] slab per range; the slabs are added in index order (in the prologue of the next
 * kernel).  The two size entries return 0 for sizes the calls refuse. */
int    yr_bn_train_chunk(long long pixels, int C);
size_t yr_bn_train_workspace_bytes(long long pixels, int C);
int yr_bn_train_forward(const float* z, int z_ld, const float* gamma, const float* beta, long long pixels, int C,
                        float eps, float momentum, int act,
                        float* a, int a_ld, float* mean /*[C]*/, float* invstd /*[C]*/,
                        float* moving_mean /*[C] in place, or null*/, float* moving_var /*[C] in place; both or neither*/,
                        void* workspace, size_t workspace_bytes, void* stream);
int yr_bn_train_backward(const float* da, int da_ld, const float* z, int z_ld, const float* gamma, const float* beta,
                         const float* mean, const float* invstd, long long pixels, int C, int act,
                         float* dz /*or null: not computed*/, int dz_ld, float* dgamma /*[C]*/, float* dbeta /*[C]*/,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- the operators that fuse maps of different scales, forward and backward (yolo3/model.py:117-168, the RFCR module: UpSampling2D,
 * MaxPooling2D and the learned WeightedSum of four maps in front of a separable convolution, three Concatenates behind it; the FPN and
 * PANet passes, model.py:240-323, use the same two resampling operators); added under ABI 9 (additive).  csrc/fusegrad.hip has the kernels'
 * forms, tests/fusegrad_ref.py is the definition (the reference's backward is TensorFlow's tape).  The conventions of the entries above
 * hold: float32, maps [B][H][W][ld] or rows [pixels][ld] with C <= ld channels taken (pad columns neither read nor written), 4-byte
 * alignment, no float atomics, nothing read before the call wrote it, every named output element written and nothing else, the same call
 * gives the same bytes, every operation one IEEE float32 operation in the order written.  YR_ERR_ARG, nothing written, for sizes outside
 * the contract, a leading dimension below C, a null pointer, byte offsets beyond 2^63, a short or misaligned workspace.  Concatenation
 * (model.py:166-168) has no arithmetic and no entry: it is a choice of pointer and leading dimension. */
/* MaxPooling2D((k, k)) (model.py:139-144, :161, :166; stride k, 'valid'), k in {2, 4}: x [B][H][W], y and dy [B][OH][OW], OH = H div k,
 * OW = W div k, H, W >= k, B * H * W < 2^40.  Rows and columns of x at and past OH * k / OW * k are not read.
 *   forward   the window is scanned in row-major order: m = x[oy k][ox k]; a later element replaces m only when it is STRICTLY greater;
 *             y[oy][ox] = m.
 *   backward  takes dy and the forward's input x; no index map is kept.  The forward's scan is repeated; dx at the FIRST position that
 *             holds the maximum receives dy[oy][ox], every other position of the window and every position of the trailing strip
 *             (rows >= OH k, columns >= OW k) receives +0.  Each dx[b][0..H)[0..W)[0..C) is written exactly once.
 * The tie rule is TensorFlow's MaxPoolGrad as restated from memory (torch.max_pool2d follows the same rule): UNPINNED BY THE REFERENCE,
 * which has no backward code and whose framework is not available where this is tested.  -0 and +0 compare equal: the first of them
 * wins.  Non-finite inputs are outside the contract.  One launch each. */
int yr_maxpool_forward(const float* x, int x_ld, int B, int H, int W, int C, int k, float* y, int y_ld, void* stream);
int yr_maxpool_backward(const float* dy, int dy_ld, const float* x, int x_ld, int B, int H, int W, int C, int k,
                        float* dx, int dx_ld, void* stream);
/* UpSampling2D() (model.py:161, :168; nearest neighbour, x2): x and dx [B][H][W], y and dy [B][2H][2W]; H and W are the SMALL map's,
 * B * H * W < 2^38.
 *   forward   y[2i + a][2j + b] = x[i][j] for a, b in {0, 1}.
 *   backward  dx[i][j] = ((dy[2i][2j] + dy[2i][2j + 1]) + dy[2i + 1][2j]) + dy[2i + 1][2j + 1]: three float32 additions in this order.
 * One launch each. */
int yr_upsample2_forward(const float* x, int x_ld, int B, int H, int W, int C, float* y, int y_ld, void* stream);
int yr_upsample2_backward(const float* dy, int dy_ld, int B, int H, int W, int C, float* dx, int dx_ld, void* stream);
/* WeightedSum of exactly four maps (model.py:117-137, :161), rows [pixels][ld], alpha [4] on the device; 1 <= pixels < 2^40,
 * 1 <= C <= 2^30.
 *   forward   y = ((alpha[0] x0 + alpha[1] x1) + alpha[2] x2) + alpha[3] x3: each product rounded, then the sums left to right - the
 *             order of model.py:134 and of YR_OP_WSUM, whose float32 bits it returns.  One launch.
 *   backward  dx_i = alpha[i] * dy; each of the four dx pointers may be null: not computed.  dalpha[i] = sum_{p, c} dy[p][c] * x_i[p][c],
 *             each term one rounded product added by one rounded addition; dalpha may be null: not computed, then no x_i is read (they
 *             may be null) and the workspace is not touched (it may be null).  With everything null nothing is launched.
 *             dalpha is a two-stage sum: stage 1 gives every workgroup a contiguous range of yr_wsum_chunk(pixels, C) pixels - a
 *             function of its arguments only -, writes the dx_i of the range and one slab of four floats to the workspace (device,
 *             16-byte aligned, yr_wsum_workspace_bytes(pixels, C) bytes, contents before the call do not matter); within a workgroup
 *             the order is fixed (csrc/fusegrad.hip: a lane's products in order from +0, the lanes of a wave by a butterfly, the
 *             waves in order); stage 2 adds the slabs in index order.  Two launches with dalpha, one without.
 * The two size entries return 0 for sizes the calls refuse. */
int    yr_wsum_chunk(long long pixels, int C);
size_t yr_wsum_workspace_bytes(long long pixels, int C);
int yr_wsum_forward(const float* x0, int x0_ld, const float* x1, int x1_ld, const float* x2, int x2_ld, const float* x3, int x3_ld,
                    const float* alpha /*device [4]*/, long long pixels, int C, float* y, int y_ld, void* stream);
int yr_wsum_backward(const float* dy, int dy_ld, const float* x0, int x0_ld, const float* x1, int x1_ld, const float* x2, int x2_ld,
                     const float* x3, int x3_ld, const float* alpha /*device [4]*/, long long pixels, int C,
                     float* dx0 /*or null*/, int dx0_ld, float* dx1 /*or null*/, int dx1_ld, float* dx2 /*or null*/, int dx2_ld,
                     float* dx3 /*or null*/, int dx3_ld, float* dalpha /*device [4], or null*/,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- the squeeze-excite block, forward and backward (yolo3/efficientnet.py:406-438: reduce_mean over the map, the 1x1 convolution
 * <name>_se_reduce with bias, Swish, the 1x1 convolution <name>_se_expand with bias, sigmoid, Multiply; every MBConv of the EfficientNet
 * backbones and of the six head blocks, yolo3/model.py:91-115, runs one with se_ratio 0.25); added under ABI 9 (additive).
 * csrc/segrad.hip has the kernels' forms, tests/segrad_ref.py is the definition (the reference's backward is TensorFlow's tape: its
 * rules for reduce_mean, Conv2D + bias, x sigmoid(x), sigmoid and Multiply, restated).  The conventions of the entries above hold:
 * float32, maps [B][H][W][ld] with C <= ld channels taken (pad columns neither read nor written), 4-byte alignment, no float atomics,
 * nothing read before the call wrote it, every named output element written and nothing else, the same call gives the same bytes.
 * x, y, dy, dx are maps, N = H * W pixels an image; w1 [C][R] (the Keras kernel [1,1,C,R]), b1 [R], w2 [R][C], b2 [C], m [B][C],
 * z1 [B][R], g [B][C], dw1, db1, dw2, db2 (the shapes of w1, b1, w2, b2) are dense.  B, H, W >= 1, B * H * W < 2^40, 1 <= C <= 4096,
 * 1 <= R <= 1024; the workspace (device, 16-byte aligned, yr_se_workspace_bytes(B, H * W, C, R) bytes: enough for either call) may hold
 * anything before the call.  YR_ERR_ARG, nothing written, for anything else, a null pointer where none is allowed, a leading dimension
 * below C, byte offsets beyond 2^63, a short or misaligned workspace, some but not all of dw1, db1, dw2, db2.  Every operation is one
 * IEEE float32 operation in this order, nothing contracted (the only fused multiply-adds are those inside the pinned exp of sigmoid):
 *   forward   S[b][c] = sum_p x[b][p][c];  m = S / (float)N;  z1[b][r] = b1[r] + sum_c m[b][c] * w1[c][r];  h = z1 * sigmoid(z1)
 *             (YR_ACT_SWISH of the forward kernels);  z2[b][c] = b2[c] + sum_r h[b][r] * w2[r][c];  g = sigmoid(z2);  y = x * g[b][c].
 *             Writes y, m, z1, g.  3 launches.
 *   backward  takes dy, x, w1, w2 and the forward's m, z1, g; h is recomputed from z1 by the forward's operations (the same bits).
 *             dg[b][c] = sum_p dy[b][p][c] * x[b][p][c] (each term one rounded product, added by one rounded addition);  t = 1.0f - g;
 *             u = g * t;  dz2 = dg * u;  dh[b][r] = sum_c dz2[b][c] * w2[r][c];  dz1 = dh * (sg * (1.0f + z1 * (1.0f - sg))),
 *             sg = sigmoid(z1) (the Swish rule of yr_bn_act_backward);  dm[b][c] = sum_r dz1[b][r] * w1[c][r];  q = dm / (float)N;
 *             dx = dy * g[b][c] + q[b][c] (a rounded product, then a rounded addition);  db2[c] = sum_b dz2[b][c];
 *             dw2[r][c] = sum_b h[b][r] * dz2[b][c];  db1[r] = sum_b dz1[b][r];  dw1[c][r] = sum_b m[b][c] * dz1[b][r] - every sum
 *             over the batch in increasing b, the first term image 0's own.  dx may be null: not computed, its map pass not launched.
 *             dw1, db1, dw2, db2 are all given or all null: when null the batch sums are not computed.  4 launches, 3 with dx or the
 *             parameters alone, none with neither.
 * The orders of the sums.  A sum over the pixels has two stages: stage 1 gives every workgroup a contiguous range of
 * yr_se_chunk(B, H * W, C) pixels of ONE image (a function of H * W and C only: an image alone is summed as inside a batch) and writes
 * one [C] slab per range; within a range the pixels are dealt to PP = 256 / Cb lanes a channel in turn (Cb = ceil(C / ceil(C / 64))),
 * a lane adds its terms in pixel order from +0, the lanes are added in order from +0; stage 2 adds an image's slabs in index order from
 * +0.  The sums of the two 1x1 convolutions and of their backward are plain products and sums in the orders csrc/segrad.hip's header
 * gives (`fc`: slices of the inputs in order, then bias + the slices in order; `fct`: 64 interleaved lane sums folded by halves).
 * The two size entries return 0 for sizes the calls refuse. */
long long yr_se_chunk(int B, long long N, int C);
size_t    yr_se_workspace_bytes(int B, long long N, int C, int R);
int yr_se_forward(const float* x, int x_ld, const float* w1 /*[C][R]*/, const float* b1 /*[R]*/, const float* w2 /*[R][C]*/,
                  const float* b2 /*[C]*/, int B, int H, int W, int C, int R, float* y, int y_ld, float* m /*[B][C]*/,
                  float* z1 /*[B][R]*/, float* g /*[B][C]*/, void* workspace, size_t workspace_bytes, void* stream);
int yr_se_backward(const float* dy, int dy_ld, const float* x, int x_ld, const float* w1, const float* w2, const float* m,
                   const float* z1, const float* g, int B, int H, int W, int C, int R, float* dx /*or null*/, int dx_ld,
                   float* dw1 /*[C][R]*/, float* db1 /*[R]*/, float* dw2 /*[R][C]*/, float* db2 /*[C]; all four or none*/,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- the 1x1 operators at any width up to 1024 channels on either side: the neck and the heads behind the RFCR module are wider than
 * yr_linear_forward / _dgrad / _wgrad take (model.py:226-258: td1_conv 216..480 -> 512, td2_conv 424..576 -> 256, td3_conv 248..272 ->
 * 128, bu1_conv 331 -> 512; model.py:104-111: the projections 512 -> anchors * (classes + 5)), and code/train.py:150-171 trains all of
 * them.  Added under ABI 9 (additive: the narrow entries are unchanged, their 256-channel refusal included).  csrc/linearwide.hip has
 * the kernels' forms and the order of every sum.  The argument lists, the conventions (float32, rows row-major over pixels with a
 * leading dimension in floats, Wt[cout][kp] with kp = round_up(cin, 4) and pad columns never read, 4-byte alignment, no float atomics,
 * nothing read before the call wrote it, every named output element written and nothing else, the same call gives the same bytes)
 * and the refusals (YR_ERR_ARG, nothing launched or written: a null pointer, ld below the channels taken, a misaligned pointer, byte
 * offsets beyond 2^63, a workspace that is short or not 16-byte aligned, sizes outside 1 <= cin, cout <= 1024, 1 <= pixels < 2^40; the forward
 * and the input gradient, one workgroup per 64 pixels, refuse more than 2^37 - 64 pixels, as the narrow twins do) are those of the
 * narrow twins.  The narrow widths are accepted as well and give the narrow entries' bytes in all three entries. */
/* model.py:29,100,111 (a bias-free 1x1 Conv2D): y[p][co] = sum_k x[p][k] * wt[co][k], the activations read once per 256 output
 * channels.  At cin, cout <= 256 the bytes of yr_linear_forward.  One launch. */
int yr_linear_wide_forward(const float* x, int x_ld, const float* wt /*[cout][kp]*/, long long pixels, int cin, int cout,
                           float* y, int y_ld, void* stream);
/* d loss / d x of that layer (tape.gradient, yolo3/train.py:39): dx[p][ci] = sum_co dy[p][co] * wt[co][ci], dy read once per 256 input
 * channels.  At cin, cout <= 256 the bytes of yr_linear_dgrad.  One launch. */
int yr_linear_wide_dgrad(const float* dy, int dy_ld, const float* wt /*[cout][kp]*/, long long pixels, int cin, int cout,
                         float* dx, int dx_ld, void* stream);
/* d loss / d Wt of that layer (yolo3/train.py:39): dwt[co][ci] = sum_p dy[p][co] * x[p][ci], two launches like yr_linear_wgrad: stage 1
 * gives every workgroup a contiguous range of yr_linear_wide_wgrad_chunk(pixels, cin, cout) pixels - the least multiple of 16 that is
 * at least 64, ceil(cout * kp / (cin + cout)) and ceil(pixels / 1024): a function of its three arguments only - and 128 x 128 channels,
 * and writes one [cout][kp] slab per range; stage 2 adds the slabs in index order and writes EVERY element of dwt, pad columns as +0.
 * Where cin and cout are both at most 256 the call IS yr_linear_wgrad - its chunk, its workspace size, its bytes (one 128 x 128 block
 * gains nothing from the wide stage 1) -, and the two size entries return the narrow ones' values.  They return 0 for sizes the call
 * refuses. */
int    yr_linear_wide_wgrad_chunk(long long pixels, int cin, int cout);
size_t yr_linear_wide_wgrad_workspace_bytes(long long pixels, int cin, int cout);
int    yr_linear_wide_wgrad(const float* x, int x_ld, const float* dy, int dy_ld, long long pixels, int cin, int cout,
                            void* workspace /*device*/, size_t workspace_bytes, float* dwt /*[cout][kp]*/, void* stream);

/* ---- the network entry as a training operator: the dense 3 x 3 convolution of 1..4 -> 1..64 channels every backbone starts with
 * (code/yolo3/model.py:180,193: MobileNetV2's Conv1; code/yolo3/efficientnet.py: stem_conv; code/train.py:150-216 trains it with every
 * other layer, tape.gradient at yolo3/train.py:39).  Added under ABI 9 (additive: no struct or existing entry changed).
 * csrc/stemgrad.hip has the kernels' forms, tests/stemgrad_ref.py is the definition.  The conventions of the depthwise training
 * entries hold: float32 maps [B][H][W][ld] with 4-byte alignment, stride in {1, 2}, explicit pad_top, pad_left in 0..2 and the
 * output size (OH, OW), which must be floor((H + pad_top + pad_bottom - 3) / stride) + 1 for some pad_bottom in 0..2 (columns
 * alike); no float atomics, nothing read before the call wrote it, every named output element written and nothing else (pad channels
 * [cin, x_ld) and [cout, y_ld) are neither read nor written), the same call gives the same bytes.  YR_ERR_ARG with a message, nothing
 * launched or written, for a null or misaligned pointer, cin outside 1..4, cout outside 1..64, a stride or pad outside the contract,
 * a leading dimension below the channels, an output size the geometry does not give, B, H, W, OH or OW above 65535, a short or
 * misaligned workspace.  The weight w is the Keras kernel [3, 3, cin, cout] as it lies in memory: row r = (ky * 3 + kx) * cin + ci,
 * cout dense floats a row.
 * THE ORDER: one fmaf per term and nothing else, every chain from +0, taps row-major and channels innermost.
 *   forward  y[b][oy][ox][co]: for ky, for kx, for ci: acc = fmaf(x[b][oy s - pad_top + ky][ox s - pad_left + kx][ci], w[r][co], acc)
 *   dgrad    dx[b][iy][ix][ci]: for ky, for kx with iy + pad_top - ky = oy s and ix + pad_left - kx = ox s, for co:
 *            acc = fmaf(dy[b][oy][ox][co], w[r][co], acc).  Every dx[..][0..cin) is written: +0 where no window reaches.
 *   A tap outside the map, or whose output pixel does not exist, is SKIPPED - no operation, not an fmaf with a zero: a chain that
 *   is -0 stays -0.
 *   wgrad    dw[r][co] = sum_{b,oy,ox} dy[b][oy][ox][co] * x[b][oy s - pad_top + ky][ox s - pad_left + kx][ci], two launches: stage 1
 *            cuts the B * OH output rows into chunks of yr_conv3x3_wgrad_chunk(B, OH, OW, cin, cout) rows - the least number that
 *            gives a chunk 256 pixels and leaves at most 2048 chunks: a function of its arguments only - and writes one
 *            [9 cin][cout] slab per chunk.  Within a chunk, pixels numbered i = 0, 1, .. in (row, column) order, NS = 4 (cout <= 28),
 *            2 (cout <= 56) or 1 partial sums s take the pixels i = s, s + NS, .. in order, acc = fmaf(dy, x, acc), skipped taps as
 *            above, and are added as ((s0 + s1) + s2) + s3.  Stage 2 adds the slabs in index order, the first term slab 0 itself,
 *            and writes every dw element.  The workspace (16-byte aligned) holds the slabs; its contents before the call do not
 *            matter.  The two size entries return 0 for sizes the call refuses. */
int    yr_conv3x3_forward(const float* x, int x_ld, const float* w /*[9*cin][cout]*/, int B, int H, int W, int cin, int cout, int stride,
                          int pad_top, int pad_left, int OH, int OW, float* y, int y_ld, void* stream);
int    yr_conv3x3_dgrad(const float* dy, int dy_ld, const float* w /*[9*cin][cout]*/, int B, int H, int W, int cin, int cout, int stride,
                        int pad_top, int pad_left, int OH, int OW, float* dx, int dx_ld, void* stream);
int    yr_conv3x3_wgrad_chunk(int B, int OH, int OW, int cin, int cout);
size_t yr_conv3x3_wgrad_workspace_bytes(int B, int OH, int OW, int cin, int cout);
int    yr_conv3x3_wgrad(const float* x, int x_ld, const float* dy, int dy_ld, int B, int H, int W, int cin, int cout, int stride,
                        int pad_top, int pad_left, int OH, int OW, void* workspace /*device*/, size_t workspace_bytes,
                        float* dw /*[9*cin][cout]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YOLORET_HIP_H */
