/*
 * f8net.h — C ABI of libf8net.so: the MI355X (gfx950) fixed-point-8 integer inference path.
 *
 * The reference (snap-research/F8Net) has no FFI: its `int_op_only` forward is plain nn.Module
 * composition over int32 CPU tensors.  This header declares what a binding for
 * that path binds instead; every entry point cites the reference call site it replaces
 * (paths relative to /root/reference).  INTEGRATION.md shows the reference-side stubs.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  Status: 0 = ok, < 0 = f8_status.
 *     No exception crosses the ABI; f8_last_error() gives the message for the calling thread.
 *   - All `*_dev` pointers are device (HBM) pointers owned by the caller.  `stream` is a
 *     hipStream_t passed as void*; every call is asynchronous on it and never synchronises.
 *   - Tensors at the boundary use the reference's format: int32, NCHW contiguous, values of
 *     activations in 8-bit range where the reference guarantees it.  The fraction length the
 *     reference carries as the Python attribute `output_fraclen` is an explicit integer here.
 *   - Inside a net, activations live as NHWC int8 / int32 in an arena owned by the handle.
 *   - Thread safety: distinct handles are independent; one handle must not be run concurrently.
 */
#ifndef F8NET_H
#define F8NET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define F8NET_VERSION 200

typedef enum f8_status {
    F8_OK = 0,
    F8_ERR_INVALID = -1,      /* argument the reference would assert on, or malformed graph */
    F8_ERR_UNSUPPORTED = -2,  /* legal in the reference, not built here (e.g. 1 < groups < cin on a handle whose option `grouped` is 0, the default; a depthwise kernel of 9) */
    F8_ERR_HIP = -3,          /* HIP runtime error (message in f8_last_error) */
    F8_ERR_NOMEM = -4,
    F8_ERR_STATE = -5         /* call out of order (e.g. run before finalize) */
} f8_status;

const char* f8_status_string(int status);
const char* f8_last_error(void);
int f8_version(void);
/* Number of visible HIP devices (0 without a GPU; never fails). */
int f8_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Op-level seam: element-wise pieces of IntBlock.forward on int32 device tensors (any shape,
 * n elements, contiguous).
 * ------------------------------------------------------------------------------------------ */

/* int_op_only_fix_quant(input, 8, dst_fl, src_fl, signed)  — models/fix_quant_ops.py:90-114.
 * Shift by n = src_fl - dst_fl with round-half-to-even (n > 0) or left shift (n <= 0), then
 * clamp to [-127,127] (signed) or [0,255].  F8_ERR_INVALID where the reference asserts
 * (dst_fl outside [0, 8 - signed], :91-98) or |n| > 30.  src == dst allowed. */
int f8_requant_i32(const int32_t* src_dev, int32_t* dst_dev, size_t n,
                   int src_fl, int dst_fl, int is_signed, void* stream);

/* Input quantisation of forward_loss as a stand-alone op — fix_train.py:683-692:
 *   normalize == 0: dst = round_half_even(255 * src)  (fl, is_signed ignored; output fraclen 8; no clamp, as in the reference)
 *   normalize != 0: dst = clamp(round_half_even(src * 2^fl), [-127,127] if is_signed else [0,255])
 * F8_ERR_INVALID where fix_quant asserts (fl outside [0, 8 - signed], fix_quant_ops.py:66-71). */
int f8_quantize_input_f32(const float* src_dev, int32_t* dst_dev, size_t n, int normalize, int fl, int is_signed, void* stream);

/* Scoring of forward_loss — fix_train.py:697-704: correct_dev[k][n] = 1.0f if target n is among the ks[k] largest
 * logits of image n, else 0 (the rows the reference concatenates behind the loss).  Equal logits rank by lower class
 * index.  logits_dev: float32 [N, classes]; target_dev: int64 [N]; ks: host array of nk <= 8 values. */
int f8_topk_correct_f32(const float* logits_dev, const int64_t* target_dev, int N, int classes,
                        const int* ks, int nk, float* correct_dev, void* stream);

/* nn.ReLU on int32 — models/fix_resnet.py:39,77.  In place. */
int f8_relu_i32(int32_t* x_dev, size_t n, void* stream);

/* Residual align-add-clamp — models/fix_resnet.py:40-54,63-76; fix_mobilenet_v2.py:34-48:
 * the operand with the smaller fraclen is shifted left, res += x (wrapping), clamp to
 * [-(2^31-1), 2^31-1].  res updated in place; *out_fl (host, may be NULL) = max(res_fl, x_fl). */
int f8_add_align_i32(int32_t* res_dev, const int32_t* x_dev, size_t n,
                     int res_fl, int x_fl, int* out_fl, void* stream);

/* ------------------------------------------------------------------------------------------
 * Net-level seam: IntModel.forward — models/fix_resnet.py:352-383,
 * fix_mobilenet_v2.py:207-241, fix_mobilenet_v1.py:120-147 — as a graph of integer ops built
 * once from the exported parameters (state_dict of `Model.int_model()`, fix_resnet.py:526-544)
 * and run many times.  The same builder with one conv / pool / linear node is the op-level
 * replacement for `layer_(res)` (fix_resnet.py:34,59), `self.head[...]` (:356-359),
 * FXQAvgPool2d (fix_quant_ops.py:126-134) and `self.classifier(x)` (:383).
 *
 * Tensor ids are small non-negative ints returned by the builder calls (< 0 = f8_status).
 * A tensor id names the int32-valued tensor the reference would hold at that point, together
 * with its output_fraclen; how it is materialised (int8 for conv consumers — the consumer's
 * int_op_only_fix_quant is fused into the producer's epilogue — int32 for residual / pooling
 * consumers) is decided by f8_net_finalize.
 * ------------------------------------------------------------------------------------------ */

typedef struct f8_net f8_net;

typedef struct f8_conv_desc {
    int32_t cin, cout;
    int32_t kernel;        /* square kernels: 1, 3, 7 in the reference nets (rectangular ones, per-axis strides and pads: f8_net_conv_rect) */
    int32_t stride, pad;
    int32_t groups;        /* 1 or cin (depthwise, cout == cin) — fix_quant_ops.py:373-390.  Depthwise: kernel 3, 5 or 7,
                              stride 1 or 2, 0 <= pad <= kernel / 2; anything else depthwise is F8_ERR_UNSUPPORTED.
                              1 < groups < cin (grouped, the int nn.Conv2d of fix_quant_ops.py:680-714): F8_ERR_UNSUPPORTED unless the
                              handle's option `grouped` is 1 or 2, set BEFORE this call; then any geometry a plain conv takes, and
                              groups must divide cin and cout (F8_ERR_INVALID) */
    int32_t weight_fl;     /* buffer `weight_fraclen` (fix_quant_ops.py:710) */
    int32_t input_fl;      /* buffer `input_fraclen`  (fix_quant_ops.py:711) */
    int32_t input_signed;  /* attr `input_symmetric`  (fix_quant_ops.py:709) */
    int32_t quant_input;   /* 1: int_op_only_fix_quant(src -> input_fl) precedes the conv
                              (fix_resnet.py:30-34); 0: src already holds input_fl-format
                              integers (head conv, fix_resnet.py:356-358; op-level use) */
    int32_t relu;          /* an nn.ReLU follows the conv (int_block, fix_resnet.py:314) */
} f8_conv_desc;

typedef struct f8_linear_desc {
    int32_t in_features, out_features;
    int32_t weight_fl, input_fl, input_signed, quant_input;
} f8_linear_desc;

f8_net* f8_net_create(void);
void f8_net_destroy(f8_net* net);

/* Network input: int32 NCHW [N,C,H,W] at run time, tagged with `fraclen` as forward_loss does
 * (fix_train.py:683-692: u8 0..255 at fraclen 8, or signed at head.input_fraclen). */
int f8_net_input(f8_net* net, int C, int H, int W, int fraclen);

/* Integer conv built by ReLUClipFXQConvBN.int_conv (fix_quant_ops.py:680-714).
 * weight: host int32 [cout, cin/groups, k, k] (values must fit int8); bias: host int32 [cout]
 * (32-bit fixed point at fraclen input_fl + weight_fl, :612-614) or NULL.
 * Result tensor: fraclen weight_fl + input_fl (fix_resnet.py:35-37). */
int f8_net_conv(f8_net* net, int src, const f8_conv_desc* desc,
                const int32_t* weight_host, const int32_t* bias_host);

/* The same conv with `dilation` between its taps (int_conv passes dilation = self.conv.dilation into the int nn.Conv2d, fix_quant_ops.py:686):
 * output size (H + 2 pad - dilation (kernel - 1) - 1) / stride + 1; weights as f8_net_conv ([cout, cin/groups, k, k], the k x k real taps).
 * f8_net_conv is the dilation == 1 call of this function.  Accepted for 1 <= dilation <= 64: plain convs (groups == 1) of any geometry
 * f8_net_conv takes (kernel == 1: dilation is normalised to 1), on conv_igemm_kernel, a launch of its own (conv3x3s1d2_t128x64x64[_res]:) that may
 * carry the residual join; depthwise convs of kernel 3 with pad <= dilation, stride 1 / 2 (dwconv3x3s1d2:, f8_dwk.hip); grouped convs on a handle
 * with option grouped >= 1, always as the dense expansion (gconv3x3s1d2_dense:).  A dilated conv joins no fused block or chain launch.
 * F8_ERR_INVALID: dilation < 1, or an empty output; F8_ERR_UNSUPPORTED: dilation > 64, or a depthwise kernel of 5 / 7 with dilation > 1. */
int f8_net_conv_dilated(f8_net* net, int src, const f8_conv_desc* desc, int dilation,
                        const int32_t* weight_host, const int32_t* bias_host);

/* The same conv with a rectangular kernel, a stride per axis and four pads (nn.Conv2d with tuple kernel_size / stride / dilation behind an explicit
 * zero pad; ONNX Conv with kernel_shape, strides and pads = [top, left, bottom, right]): the 1x7 / 7x1 of Inception-v3, the 3x1 / 1x3 (dilated) of
 * ERFNet, the depthwise 1xk / kx1 strips of SegNeXt, the SAME padding (0, 0, 1, 1) of TF-derived stride-2 convs.
 * `desc` means what it means for f8_net_conv, but its `kernel`, `stride` and `pad` must be 0 (F8_ERR_INVALID): the geometry comes from `geom` only.
 * weight: host int32 [cout, cin/groups, kh, kw] (int8 values), the kh x kw real taps; bias as f8_net_conv.
 * Result: [cout, P, Q], P = (H + pad_top + pad_bottom - dilation (kh - 1) - 1) / stride_h + 1 (floor), Q alike from W, pad_left / pad_right, kw and
 * stride_w; fraclen weight_fl + input_fl.  In wrapping int32 arithmetic
 *   out[n, co, p, q] = b[co] + sum x_q[n, ci, p stride_h - pad_top + dilation r, q stride_w - pad_left + dilation s] * w[co, ci, r, s]
 * over ci of the group, r < kh, s < kw, a tap outside the image reading 0; x_q, relu and the bias as f8_net_conv.
 * Not a new op where it is square: kh == kw, stride_h == stride_w and four equal pads record exactly the node f8_net_conv_dilated records (the same
 * plan, tokens, fusions and kernels); kh == kw == 1 normalises the dilation to 1.
 * Accepted, plain (groups == 1): 1 <= kh, kw <= 31, strides >= 1, 1 <= dilation <= 64, each pad from 0 to its axis' extent - 1 (extent =
 * dilation (k - 1) + 1: a 1-wide axis takes no pad), a non-empty output.  One launch of conv_igemm_kernel that may carry the residual join, as a
 * dilated conv: `conv1x7s1_t64x64x64[_res]:`, `conv3x1s1d2_...:`, `conv3x5s2x1_...:` where the strides differ.  It joins no fused block or chain.
 * Accepted, depthwise (groups == cin == cout): strips only — one of kh / kw is 1, the other k with 3 <= k <= 31 —, dilation 1, stride 1 or 2 (the
 * same on both axes), pads <= k - 1 on the strip axis and 0 on the unit axis: `dwconv1x21s1:` / `dwconv21x1s1:` (f8_dwk.hip: dwstrip_dot4_kernel for
 * int8-only results at stride 1 under option dwk_dot4, else dwconvk_kernel).
 * F8_ERR_UNSUPPORTED (the message names the geometry): every other depthwise rectangle (kh, kw both > 1 and unequal, a dilated strip, per-axis
 * strides), grouped rectangular convs (1 < groups < cin, whatever option `grouped` says).  F8_ERR_INVALID: a null desc / geom, desc->kernel / stride /
 * pad != 0, a kernel, stride, pad or dilation outside the rules above, an empty output.  F8_ERR_STATE after finalize.
 * Not built: rectangular pools and transposed convs; grouped rectangular convs; general kh x kw, dilated or per-axis-strided depthwise convs; a
 * fused 1xk -> kx1 pair; an LDS-patch kernel for strips. */
typedef struct f8_conv_geom {
    int32_t kh, kw;
    int32_t stride_h, stride_w;
    int32_t pad_top, pad_left, pad_bottom, pad_right;
    int32_t dilation;      /* one spacing for both axes, as f8_net_conv_dilated */
} f8_conv_geom;
int f8_net_conv_rect(f8_net* net, int src, const f8_conv_desc* desc, const f8_conv_geom* geom,
                     const int32_t* weight_host, const int32_t* bias_host);

/* Transposed convolution (the learned upsampler: nn.ConvTranspose2d(k=2, s=2) of a U-Net decoder, 4x4 / 2 / pad 1 of FCN, CenterNet and pose heads,
 * 3x3 / 2 / pad 1 / output_padding 1 of encoder-decoders).  The reference names a ReLUClipFXQConvTransposeBN (fix_quant_ops.py:9) but defines no such
 * class, so the integer semantics are fixed here: those of int_conv applied to nn.ConvTranspose2d.
 * `desc` is the f8_conv_desc of f8_net_conv and every field means what it means there (quant_input, input_fl, input_signed, weight_fl, relu, kernel,
 * stride, pad; groups must be 1).  weight: host int32 [cin, cout, k, k] — the layout of nn.ConvTranspose2d.weight and of ONNX ConvTranspose's W —
 * values must fit int8; bias: host int32 [cout] at fraclen input_fl + weight_fl, or NULL.
 * Result: [cout, P, Q] with P = (H - 1) stride - 2 pad + kernel + output_padding (Q alike from W), fraclen weight_fl + input_fl, and in wrapping
 * int32 arithmetic, as for a conv,
 *   out[n, co, oh, ow] = b[co] + sum x_q[n, ci, ih, iw] * w[ci, co, kh, kw]
 *                        over ci, kh, kw with oh + pad - kh = stride * ih, 0 <= ih < H  and  ow + pad - kw = stride * iw, 0 <= iw < W
 * where x_q is the source behind the consumer requantisation (quant_input) or the source itself; a ReLU follows when desc->relu is set.  The same
 * function three ways: the scatter form (every input pixel adds x * w[.., kh, kw] at (stride ih - pad + kh, ..)), the per-phase gather above, and the
 * plain conv with pad' = kernel - 1 - pad and flipped, in / out-swapped weights over the zero-stuffed input (stride - 1 zeros between pixels,
 * output_padding zero rows / columns at the bottom / right) — all equal to torch.nn.functional.conv_transpose2d.
 * Accepted: 1 <= kernel <= 8, 1 <= stride <= 4, 0 <= pad <= kernel - 1, 0 <= output_padding < stride, groups == 1.
 * F8_ERR_INVALID: output_padding < 0 or >= stride, an empty output (P or Q < 1), a weight outside int8, cin != the source's channels, whatever the
 * consumer format refuses (f8_net_conv); F8_ERR_UNSUPPORTED: kernel > 8, stride > 4, pad > kernel - 1, groups != 1, a result past the 2 GiB-per-tensor
 * bound; F8_ERR_STATE after finalize.
 * stride == 1 is not a new op: it is recorded as the equivalent plain conv node (flipped, swapped weights, pad' = kernel - 1 - pad) and plans, fuses
 * and names itself as any f8_net_conv does.  stride >= 2 is one launch of f8::deconv_kernel<1 / 2> (f8_deconv.hip), plan token `deconv{k}x{k}s{s}:`; it joins
 * no fused block or chain launch and carries no residual join (an f8_net_add whose later operand it produces stays an `add:` launch).  It reads its
 * source's int8 form as a conv does, so a tensor it reads exists in device memory: no fused launch keeps it on chip (it cuts a launch as an output
 * tap does). */
int f8_net_conv_transpose(f8_net* net, int src, const f8_conv_desc* desc, int output_padding,
                          const int32_t* weight_host, const int32_t* bias_host);

/* Residual join of IntBlock.forward (fix_resnet.py:40-54 / :63-76) [+ post_relu :77]. */
int f8_net_add(f8_net* net, int a, int b, int relu);

/* Channel concatenation (torch.cat(dim=1) of an ASPP head, an Inception module, a DenseNet block, a U-Net / FPN skip): out = concat(srcs[0] ..
 * srcs[n - 1]) along C in operand order, 2 <= n <= F8_MAX_CONCAT operands of the same H and W.  out.C = sum of C_i; fraclen = the largest operand
 * fraclen; an operand with a smaller one is aligned as the residual join aligns it (fix_resnet.py:40-54 with a zero partner): shifted left by the
 * difference with the reference's int32 wrap, clamped to +-(2^31 - 1).  No ReLU, no rounding; a consumer with quant_input = 1 requantises the result
 * from that fraclen as it does any tensor.  Returns the tensor id.  F8_ERR_INVALID: n < 2, a bad tensor id, operands of different H / W, fraclens more
 * than 31 apart; F8_ERR_UNSUPPORTED: n > F8_MAX_CONCAT, the same tensor twice; F8_ERR_STATE after finalize.
 * The plan runs it as one launch of f8_concat.hip, in one of two modes shown by its token: `concat_i8:` — the result is read in at most two int8
 * formats and by nothing else, and its values are provably far enough from 2^31 — has every operand's producer write the result's formats and
 * copies bytes; `concat_i32:` reads the operands' int32 forms and aligns in the launch (option concat_i8 = 0: always).  Same values either way.
 * A tensor read by a concat exists in device memory: no fused block or chain launch keeps it on chip (it cuts a launch as an output tap does). */
#define F8_MAX_CONCAT 8
int f8_net_concat(f8_net* net, const int* srcs, int n);

/* Upsampling (the top-down path of an FPN, a U-Net decoder, DeepLab's logits back at the input size, the broadcast of ASPP's image-pooling branch):
 * out = [C, H * scale_h, W * scale_w] from src = [C, H, W].  Both modes are exact integer functions: no rounding, no real-valued scale.
 *   F8_UP_NEAREST   1 <= scale_h, scale_w <= 256, not both 1.  out[c][P][Q] = x[c][P / scale_h][Q / scale_w] (integer division): torch's
 *                   mode='nearest' for integer scales.  The fraclen is unchanged.  A [C, 1, 1] source with scale (H, W) is a broadcast.
 *   F8_UP_BILINEAR  scale_h == scale_w == s = 2^k, k = 1 .. 4; half-pixel centres (torch's mode='bilinear', align_corners=False) scaled to integers.
 *                   Per axis of n source values, output index o = s i + j, 0 <= j < s:
 *                     j <  s / 2:  (s - 2j - 1) x[max(i - 1, 0)] + (s + 2j + 1) x[i]
 *                     j >= s / 2:  (3s - 2j - 1) x[i] + (2j + 1 - s) x[min(i + 1, n - 1)]
 *                   The weights of an axis sum to 2s; applied over H and over W every output is the exact interpolated value times 4 s^2 =
 *                   2^(2k + 2), so out.fraclen = src.fraclen + 2k + 2.  All arithmetic modulo 2^32 (the int32 wrap of f8_net_avgpool_sum), no clamp,
 *                   no rounding: a consumer with quant_input = 1 rounds once, as for any tensor.
 * Returns the tensor id.  F8_ERR_INVALID: a bad tensor id, a scale < 1 or both scales 1, an unknown mode, bilinear with an output fraclen > 32 (the
 * bound of f8_net_avgpool_sum); F8_ERR_UNSUPPORTED: a nearest scale > 256, bilinear with unequal scales or a scale outside {2, 4, 8, 16};
 * F8_ERR_STATE after finalize.
 * The plan runs it as one launch of f8_upsample.hip, its mode shown by its token: `upsample_nearest_i8:` — nearest, the result read in at most two
 * int8 formats and by nothing else — has the source's producer write those formats and replicates bytes; `upsample_nearest_i32:` /
 * `upsample_bilinear_i32:` read the source's int32 form (option upsample_i8 = 0: every nearest one).  Same values either way.
 * A tensor read by an upsample exists in device memory: no fused block or chain launch keeps it on chip (it cuts a launch as an output tap does). */
#define F8_UP_NEAREST  0
#define F8_UP_BILINEAR 1
int f8_net_upsample(f8_net* net, int src, int mode, int scale_h, int scale_w);

/* Channel slice and channel shuffle (the split and the shuffle of a ShuffleNet unit, torch.split / x[:, a:b] of a CSPNet, GhostNet or Res2Net block,
 * a head that reads part of a tensor).  Both are pure channel gathers of one map: H, W and the fraclen are the source's, and there is no
 * arithmetic at all — no shift, no clamp, no ReLU.
 *   f8_net_slice            out = src[:, first : first + channels].
 *   f8_net_channel_shuffle  torch.nn.functional.channel_shuffle: out[c] = src[(c % groups) * (C / groups) + c / groups].
 * Both return the tensor id.  F8_ERR_INVALID: a bad tensor id; a slice with first < 0, channels < 1 or first + channels > C, or of the whole
 * tensor (the identity); a shuffle with groups < 2, groups not dividing C, or groups == C (the identity).  F8_ERR_UNSUPPORTED: groups >
 * F8_MAX_CONCAT (the launch's operand table).  F8_ERR_STATE after finalize.
 * The plan runs each as one launch of f8_chanmap.hip, its mode shown by its token: `slice_i8:` / `shuffle{g}_i8:` — the result is read in at most
 * two int8 formats and by nothing else — have the source's producer write those formats and move bytes; `slice_i32:` / `shuffle{g}_i32:` read the
 * source's int32 form (option chanmap_i8 = 0: always).  A concat of `groups` operands of one width that an i8-mode shuffle alone reads emits no
 * launch: the shuffle launch reads the operands, token `concat+shuffle{g}_i8:` (option fuse_shuffle = 0: two launches).  Same values in every case.
 * A tensor read by a slice or a shuffle exists in device memory: no fused block or chain launch keeps it on chip (it cuts a launch as an output
 * tap does). */
int f8_net_slice(f8_net* net, int src, int first, int channels);
int f8_net_channel_shuffle(f8_net* net, int src, int groups);

/* Depth-to-space and space-to-depth (nn.PixelShuffle of ESPCN / EDSR / Real-ESRGAN and of a Dense Upsampling Convolution head; nn.PixelUnshuffle,
 * TResNet's SpaceToDepth stem, YOLO's reorg / Focus).  Both move values between the channel axis and the spatial axes of one map in square blocks
 * of r = block pixels a side; there is no arithmetic at all — no shift, no clamp, no ReLU — and the fraclen is the source's.
 *   f8_net_depth_to_space   [C r^2, H, W] -> [C, H r, W r].
 *                           F8_ORDER_CRD: out[n, c, h r + i, w r + j] = src[n, c r^2 + i r + j, h, w]     (torch pixel_shuffle, ONNX mode="CRD")
 *                           F8_ORDER_DCR: out[n, c, h r + i, w r + j] = src[n, (i r + j) C + c, h, w]     (ONNX DepthToSpace's default mode)
 *   f8_net_space_to_depth   [C, H r, W r] -> [C r^2, H, W], the exact inverse of the above for each order: CRD is torch pixel_unshuffle, DCR is ONNX
 *                           SpaceToDepth and TResNet's stem.
 * Both return the tensor id.  F8_ERR_INVALID: a bad tensor id, block < 2, an order other than the two, C not a multiple of r^2 (depth_to_space), H or
 * W not a multiple of r (space_to_depth).  F8_ERR_UNSUPPORTED: block > 16, a result beyond the 2 GiB per tensor of the other ops.  F8_ERR_STATE
 * after finalize.  Only square blocks.
 * The plan runs each as one launch of f8_pixmap.hip, its mode shown by its token: `d2s{r}{crd|dcr}_i8:` / `s2d{r}{crd|dcr}_i8:` — the result is read
 * in at most two int8 formats and by nothing else — have the source's producer write those formats and move bytes; `..._i32:` read the source's
 * int32 form (option pixmap_i8 = 0: always).  Same values either way.  A tensor read by one of them exists in device memory: no fused block or
 * chain launch keeps it on chip (it cuts a launch as an output tap does). */
#define F8_ORDER_DCR 0   /* ONNX DepthToSpace mode="DCR" (its default), ONNX SpaceToDepth, TResNet */
#define F8_ORDER_CRD 1   /* ONNX DepthToSpace mode="CRD" = torch pixel_shuffle / pixel_unshuffle    */
int f8_net_depth_to_space(f8_net* net, int src, int block, int order);
int f8_net_space_to_depth(f8_net* net, int src, int block, int order);

/* Fixed-point multiply of two activations and the hard gate (the scale of a squeeze-and-excitation block: SENet / SE-ResNet, MobileNet-V3, MnasNet-A1,
 * RegNetY, GhostNet; hard-swish: MobileNet-V3, LCNet).  The reference defines no such class; the semantics are fixed here in its own terms
 * (int_op_only_fix_quant, fix_quant_ops.py:91-112, on each operand; format x format -> int32, the fraction lengths add).
 *   f8_net_mul        out[n, c, h, w] = A[n, c, h, w] * B[n, c, h, w]   (b has the shape of a: element-wise, plan sub-kind "mul"), or
 *                     out[n, c, h, w] = A[n, c, h, w] * B[n, c, 0, 0]   (b is [a.C, 1, 1]: a per-image channel gate broadcast over H x W, "chmul")
 *                     with A = int_op_only_fix_quant(a, 8, a_fl, a.fraclen, a_signed) and B the same from b: the round-half-even shift and the clamp
 *                     to +-127 / 0 .. 255 every conv consumer applies.  |out| <= 255 * 255, so nothing wraps.  desc->relu: max(., 0) on the product.
 *                     out.fraclen = a_fl + b_fl, the shape is a's.  a == b is allowed: the square, in one format or in two.
 *                     Format limits are the conv's: 0 <= fl <= 8 unsigned, 0 <= fl <= 7 signed; the requant shift src.fraclen - fl lies in -31 .. 30.
 *   f8_net_hard_gate  relu6(x + 3), the numerator of hard-sigmoid, exact in fixed point:
 *                     out = clamp(x, -3 * 2^fl, +3 * 2^fl) + 3 * 2^fl,  fl = src.fraclen; shape and fraclen are the source's.  The clamp comes first, so
 *                     no int32 input overflows: INT32_MIN gives 0, INT32_MAX gives 6 * 2^fl.
 *                     The constant 1 / 6 of hard-sigmoid / hard-swish is applied NOWHERE: like the kernel^2 of f8_net_avgpool_window it is a constant
 *                     real scale that the exporter folds into the next conv's weights.
 * Compositions: the hard-sigmoid SE gate is f8_net_mul(x, f8_net_hard_gate(fc2)) with b = [C, 1, 1]; hard-swish is f8_net_mul(x, f8_net_hard_gate(x));
 * ReLU-gated or plain products are f8_net_mul alone.
 * Both return the tensor id.  F8_ERR_INVALID: a bad tensor id, a null desc, b neither of a's shape nor [a.C, 1, 1], a format outside the limits above,
 * a shift outside -31 .. 30; f8_net_hard_gate on a source with fraclen > 28 (6 * 2^fl must fit int32) or < 0.  F8_ERR_STATE after finalize.
 * NOT built: a [1, H, W] spatial broadcast, exporter support from float models.  (A true sigmoid is f8_net_table, below.)
 * The plan (f8_mul.hip).  A mul reads int8: it registers (a_fl, a_signed) on a and (b_fl, b_signed) on b exactly as a conv with quant_input = 1
 * registers its format, the producers write the forms (a third format of one tensor: a `requant:` step).  One launch, its mode shown by the token:
 * `mul_i8:` / `chmul_i8:` — the result is read in at most two int8 formats and by nothing else — writes those formats only; `mul_i32:` / `chmul_i32:`
 * writes the int32 form (a join, a pool, an output, a third format) and up to two int8 forms.  The product is bounded by 2^16: no proof about values
 * is needed.  A hard gate alone is one launch `hgate:` on its source's int32 form.  A hard gate whose ONLY reader is the b operand of one mul emits
 * no launch: the mul launch reads the gate's source in int32 and applies clamp, offset and requantisation itself, tokens `hgate+mul_i8:`,
 * `hgate+chmul_i8:` and the `_i32` pair (option fuse_hgate = 0: two launches).  Same values in every case.
 * A tensor read by a mul or a hard gate exists in device memory: no matcher counts them among a block's readers, so no fused block or chain launch
 * keeps it on chip (it cuts a launch as an output tap does). */
typedef struct f8_mul_desc {
    int32_t a_fl, a_signed;   /* format a is requantised to: int_op_only_fix_quant(a, 8, a_fl, a.fraclen, a_signed) */
    int32_t b_fl, b_signed;   /* the same for b */
    int32_t relu;             /* max(., 0) on the product */
} f8_mul_desc;
int f8_net_mul(f8_net* net, int a, int b, const f8_mul_desc* desc);
int f8_net_hard_gate(f8_net* net, int src);

/* The 256-entry table op: ANY pointwise function of an 8-bit fixed-point activation — a true sigmoid (SENet, SE-ResNet, RegNetY, EfficientNet gates;
 * pose and detection heads), swish / SiLU, Mish, GELU, leaky ReLU, tanh.  Every activation a consumer reads here is an 8-bit fixed-point value, so a
 * function of it IS a table of 256 entries, exact but for the rounding of the entries.  The reference defines no such class; the semantics are fixed
 * here in its own terms (int_op_only_fix_quant, fix_quant_ops.py:91-112, on the source):
 *   q   = int_op_only_fix_quant(src, 8, in_fl, src.fraclen, in_signed): the round-half-even shift and the clamp every conv consumer and f8_net_mul
 *         apply: 0 .. 255 unsigned, -127 .. 127 signed;
 *   out = table[q] for an unsigned format, table[q + 128] for a signed one (entry 0 of a signed table is never read).
 * The shape is the source's, out.fraclen = out_fl; no further rounding, clamp or ReLU: the entries are any int32.  The 256 entries are copied at the call.
 * Format limits are the mul's (the conv's): 0 <= in_fl <= 8 unsigned, 0 <= in_fl <= 7 signed; the shift src.fraclen - in_fl lies in -31 .. 30.
 * 0 <= out_fl <= 38: beyond 38 no 8-bit format could read the result (its shift would exceed 30).
 * Returns the tensor id.  F8_ERR_INVALID: a null desc or table, a bad tensor id, a format or shift outside the limits, out_fl outside 0 .. 38.
 * F8_ERR_STATE after finalize.  (f8net_amd/tables.py builds the entries of sigmoid, tanh, swish, mish, gelu, leaky_relu, hard_sigmoid.)
 * The plan (f8_table.hip).  A table reads int8: it registers (in_fl, in_signed) on its source as a conv with quant_input = 1 does, the producer writes
 * the form (a third format of one tensor: a `requant:` step).  Its value bound is the largest magnitude among the reachable entries.  One launch, its
 * mode by the gathers' rule, shown by the token:
 *   `table_i8:`   the result is read in at most two int8 formats and by nothing else.  At finalize the host composes one 256-BYTE table per format —
 *                 entry i = the requantisation of table[i] to that format, storage bias folded in — and the launch only moves bytes.
 *   `table_i32:`  a join, a pool, an output or a third format needs the int32 form: the launch writes it and up to two int8 forms (option table_i8 = 0:
 *                 every table runs this kernel; it then writes the int32 form only where something needs it).
 *   `table+chmul_i8:` / `table+chmul_i32:`   the sigmoid SE gate: a table that ONLY the b operand of one broadcast f8_net_mul reads, and that is no
 *                 output, emits no launch; the mul launch reads the table's source bytes and looks them up in a byte table composed for
 *                 (b_fl, b_signed) (option fuse_table: 1, the default, where the map has fewer than 2^20 values an image — the fused
 *                 launch measured slower above —, 2 always, 0 never: two launches).  Same values in every case, bit for bit.
 * The device tables live in the weight image f8_net_upload moves.  A tensor read by a table exists in device memory: no matcher counts the table among
 * a block's readers, so it cuts a chain or fused block where an output tap does.
 * NOT built: the table fused into its producer's epilogue, per-channel tables (PReLU), an element-wise table+mul (swish is itself one table),
 * exporter support from float models. */
typedef struct f8_table_desc {
    int32_t in_fl, in_signed;   /* format the source is read in: int_op_only_fix_quant(src, 8, in_fl, src.fraclen, in_signed) */
    int32_t out_fl;             /* fraction length of the entries = of the result */
} f8_table_desc;
int f8_net_table(f8_net* net, int src, const f8_table_desc* desc, const int32_t table_host[256]);

/* Head max-pool nn.MaxPool2d(k, stride, pad) via the float detour (fix_resnet.py:358-359) or
 * FXQMaxPool2d (fix_quant_ops.py:150-157); exact integer max. */
int f8_net_maxpool(f8_net* net, int src, int kernel, int stride, int pad);

/* FXQAvgPool2d int branch (fix_quant_ops.py:126-134): sum over H,W in int64, truncate to int32,
 * fraclen += shift (shiftnum = round(log2(kernel_size^2)) = 6 for the nets' FXQAvgPool2d(7)). */
int f8_net_avgpool_sum(f8_net* net, int src, int shift);

/* Windowed average pooling (DenseNet transitions, Inception's 3x3 / 1 / pad 1 branch, ResNet-D's shortcut, PSPNet's pyramid bins; ONNX AveragePool):
 * FXQAvgPool2d's int branch (fix_quant_ops.py:117-138) applied per window — sum in integers, add `shift` to the fraclen, no division, no rounding.
 * out = [C, P, Q] from src = [C, H, W], P = (H + 2 pad - kernel) / stride + 1 (floor), Q the same from W;
 *   out[c][p][q] = sum over 0 <= r, s < kernel of x[c][p stride - pad + r][q stride - pad + s], over the taps inside the map: a tap outside adds 0
 * (count_include_pad = True: the divisor kernel^2 is a constant; the real scale 2^shift / kernel^2 is folded into the neighbouring conv's weights by
 * the exporter).  All arithmetic modulo 2^32 (the int32 wrap of f8_net_avgpool_sum), no clamp, no rounding, no ReLU.  out.fraclen = src.fraclen +
 * shift; the reference's shift is round(log2(kernel^2)): 2 for 2x2 (an exact average), 3 for 3x3.
 * Accepted: 1 <= kernel <= 64, 1 <= stride <= 64, 0 <= 2 pad <= kernel (f8_net_maxpool's rule), shift >= 0.
 * Returns the tensor id.  F8_ERR_INVALID: a bad tensor id, a geometry outside the rule above, kernel == 1 with stride == 1 (the identity), P < 1 or
 * Q < 1, shift < 0, src.fraclen + shift > 32 (the reference's assert); F8_ERR_UNSUPPORTED: kernel or stride above 64; F8_ERR_STATE after finalize.
 * The GLOBAL window — kernel == H == W, pad == 0 — is not a new op: it records the node f8_net_avgpool_sum records and plans, fuses
 * (`conv1x1+avgpool:`, the `...+avgpool` chain launches) and names itself (`avgpool_sum:`) exactly as that call.  A map that is not square, or whose
 * side is not the kernel, stays windowed.
 * The plan runs every other window as one launch of f8_sumpool.hip, token `sumpool{k}x{k}s{stride}:` + the tensor's name, on the source's int32 form:
 * f8::sumpool_i32_kernel<2 / 3 / 0> (a lane per output pixel) or, for windows of 3 and more that do not overlap, f8::sumpool_wide_kernel (option sumpool_wide).  The result is
 * written in int32 and / or up to two int8 formats; a third format is a `requant:` step.
 * A tensor read by a windowed pool exists in device memory: no matcher counts the pool among a block's readers, so no fused block or chain launch keeps
 * its source on chip (it cuts a launch as an output tap does). */
int f8_net_avgpool_window(f8_net* net, int src, int kernel, int stride, int pad, int shift);

/* Integer nn.Linear built by ReLUClipFXQLinear.int_fc (fix_quant_ops.py:1165-1195);
 * src must be [C,1,1]. weight: host int32 [out, in]; bias host int32 [out] or NULL. */
int f8_net_linear(f8_net* net, int src, const f8_linear_desc* desc,
                  const int32_t* weight_host, const int32_t* bias_host);

/* Marks `src` as a network output; may be called up to F8_MAX_OUTPUTS times before f8_net_finalize, on any tensor of the graph
 * (a stage output for a detection head, the pooled vector in front of the classifier, any conv's result for a comparison with
 * the reference).  Returns the output's index: 0 for the first call (the same value as F8_OK), 1, 2, ... for the next ones.
 * F8_ERR_INVALID for a tensor that is an output of this kind already (its argmax may be one as well: f8_net_output_argmax), F8_ERR_UNSUPPORTED for one output too many, F8_ERR_STATE after finalize.
 * as_float != 0: float32 (the `.float()` of fix_resnet.py:383), else int32; every output has its own.  Layout NCHW [N,C,H,W]
 * ([N,C] for pooled / linear results).  Output 0 is what the `output_dev` of the run entries receives; the others go to the
 * buffers of f8_net_set_output_buffers.  Every output exists in device memory as int32: a fused launch that would keep the
 * tensor on chip is cut there (a tap inside a stage chain makes two launches of it, an output on the pooled tensor keeps the
 * pool out of the launch in front of it), and each further output adds one copy-out launch directly behind its producer. */
#define F8_MAX_OUTPUTS 8
int f8_net_output(f8_net* net, int src, int as_float);
/* Channel argmax as an output kind: the class map of a segmentation net, the predicted class of a classifier.
 *   out[n, h, w] = the smallest c in 0 .. C - 1 for which src[n, c, h, w] is maximal.
 * The compare is over the int32 values the tensor holds — signed, after any wrap its producer defines (a bilinear upsample wraps modulo 2^32) —, the
 * smallest index wins a tie (numpy.argmax(axis=1); torch.argmax(dim=1) as documented), and the fraclen plays no part.
 * The result is [N, H, W] ([N] for a [C, 1, 1] tensor) of uint8_t (index_bytes = F8_IDX_U8) or int32_t (F8_IDX_I32; an ONNX int64 ArgMax is returned as
 * int32).  It is an OUTPUT, not a tensor: it has no id, nothing in the net can read it, and it counts towards F8_MAX_OUTPUTS.  Returns the output's
 * index as f8_net_output does; output 0 goes to `output_dev`, later ones to the buffers of f8_net_set_output_buffers, densely packed in their element
 * type.  A tensor may carry one f8_net_output mark and one f8_net_output_argmax mark: logits and classes side by side.
 * Rules: C >= 2; F8_IDX_U8 needs C <= 255 (index 255 is then never a class: it is the poison value); F8_IDX_I32 takes any C.
 * F8_ERR_INVALID: a bad tensor id, C < 2, index_bytes neither constant, a second argmax mark on one tensor; F8_ERR_UNSUPPORTED: F8_IDX_U8 with C > 255,
 * one output too many; F8_ERR_STATE after finalize.
 * f8_net_output_info on such an output reports C = 1, the map's H and W, fraclen 0 and as_float = 0; f8_net_output_elems is H * W when it is output 0;
 * f8_net_output_kind tells the element type of any output.
 * Poison: a chain launch of the same run that gave up a halo wait (f8_net_check) turns the class map into 255 (uint8) or INT32_MIN (int32), as the value
 * outputs turn into NaN / INT32_MIN.
 * The plan: one launch of f8_argmax.hip directly behind its producer, as an output tap.  Token `argmax_u8:` / `argmax_i32:` — f8::argmax_i32t_kernel reads
 * the marked tensor's int32 form, which therefore exists in device memory: a chain or fused block is cut there exactly where an output tap cuts it, and a
 * classifier whose result is marked writes its int32 form, not the caller's buffer.  Tokens `upsample_bilinear+argmax_u8:`, `upsample_nearest+argmax_u8:`
 * and the `_i32` pair (option fuse_argmax) — the marked tensor is the result of an f8_net_upsample that NOTHING else reads (no consumer, no value output):
 * the upsample emits no launch and its result exists in no form; f8::upsample_argmax_kernel reads the upsample's SOURCE in int32 and interpolates per
 * output pixel with the weights and the wrapping arithmetic of the upsample launch, then takes the argmax of the wrapped values: bit for bit the two launches.
 * NOT built: top-k maps, softmax / confidence outputs, the argmax fused into a conv or deconv epilogue, align_corners. */
#define F8_IDX_U8  1
#define F8_IDX_I32 4
int f8_net_output_argmax(f8_net* net, int src, int index_bytes);
/* Element type of output k: 0 int32 values, 1 float32 values, 2 argmax as uint8, 3 argmax as int32.  F8_ERR_INVALID: k out of range. */
int f8_net_output_kind(const f8_net* net, int k);
/* Number of outputs marked so far. */
int f8_net_num_outputs(const f8_net* net);
/* Shape, fraclen and element type of output k (0 <= k < f8_net_num_outputs); any out-pointer may be NULL. */
int f8_net_output_info(const f8_net* net, int k, int* C, int* H, int* W, int* fraclen, int* as_float);
/* Shape and fraclen of any recorded tensor, before or after finalize (what F8Net.adaptive_avgpool sizes its windows from); NULL pointers are skipped.
 * F8_ERR_INVALID: a bad tensor id. */
int f8_net_tensor_info(const f8_net* net, int t, int* C, int* H, int* W, int* fraclen);

/* Plans the graph for batches up to max_batch: fuses requant / ReLU / residual into producer
 * epilogues, picks kernels and tiles, packs weights (host side), lays out the arena.
 * Touches no device; works without a GPU. */
int f8_net_finalize(f8_net* net, int max_batch);

/* Human-readable plan (one line per kernel launch); returns bytes needed incl. NUL. */
size_t f8_net_describe(const f8_net* net, char* buf, size_t cap);
int f8_net_num_launches(const f8_net* net);
size_t f8_net_arena_bytes(const f8_net* net);
size_t f8_net_weight_bytes(const f8_net* net);
/* Fraclen of output 0. */
int f8_net_output_fraclen(const f8_net* net);
/* Element count per image of output 0 (C*H*W of the output tensor). */
size_t f8_net_output_elems(const f8_net* net);

/* Allocates device memory on the current device and uploads packed weights.  Implicit in the
 * first f8_net_run; explicit so that callers can keep allocation out of timed regions.  The handle is bound to that
 * device: a run with another device current fails with F8_ERR_STATE (option check_device). */
int f8_net_upload(f8_net* net);

/* Runs the net on `N` images (1 <= N <= max_batch).  input_dev: int32 NCHW [N,C,H,W];
 * output_dev: float32 or int32 [N, output_elems].  Asynchronous on `stream`.
 * F8_ERR_HIP without issuing anything when a stage-chain launch of an EARLIER run of this handle gave up a halo wait (see f8_net_check): the
 * failing launch also writes its code to a host-visible word that this call reads without synchronising; runs are refused until f8_net_check
 * has collected the error (round 5).  The logits of the failed run itself are poisoned (NaN / INT32_MIN); runs issued before the failure
 * became visible are unaffected — the error word carries the failed run's tag and only that run's waits / outputs react to it. */
int f8_net_run(f8_net* net, const int32_t* input_dev, void* output_dev, int N, void* stream);

/* Same net, fed with the fp32 images forward_loss receives (fix_train.py:676-692): the input quantisation
 *   normalize == 0:  x_int = round_half_even(255 * x), fraclen 8        (fix_train.py:689-692; requires an unsigned head at fraclen 8)
 *   normalize != 0:  x_int = clamp(round_half_even(x * 2^fl), +-127 or [0,255]), fl = the head's input fraclen
 *                    (fix_train.py:683-687 through fix_quant, models/fix_quant_ops.py:64-87)
 * is applied inside the input kernel, so the int32 NCHW tensor of the reference never exists in HBM.
 * images_dev: float32 NCHW [N,C,H,W].  F8_ERR_INVALID if normalize == 0 and the net's input fraclen is not 8. */
int f8_net_run_f32(f8_net* net, const float* images_dev, int normalize, void* output_dev, int N, void* stream);

/* Same net, fed with the uint8 pixels a decoder produces (1 byte per pixel and channel instead of 4): the reference's
 * `transforms.ToTensor()` [+ `transforms.Normalize(mean, std)`] (fix_train.py:299-329) and the input quantisation of
 * forward_loss (fix_train.py:683-692) are folded into a 3 x 256 table (built per call on the host in the float32 operations
 * torch executes, so the integers are the reference's bit for bit) that the input kernel looks up while it lays the image out
 * for the head conv.  images_dev: uint8, NCHW [N,3,H,W] (nhwc == 0) or NHWC [N,H,W,3] (nhwc != 0).
 * normalize == 0: x_int = the pixel value, fraclen 8 (needs an unsigned head at fraclen 8); mean / std ignored (may be NULL).
 * normalize != 0: x_int = clamp(round_half_even(((k / 255 - mean[c]) / std[c]) * 2^fl)), fl = the head's input fraclen;
 *                 mean, std: host float[3]. */
int f8_net_run_u8(f8_net* net, const uint8_t* images_dev, int nhwc, int normalize, const float* mean, const float* std,
                  void* output_dev, int N, void* stream);

/* Optional measured tile selection: times every implicit-GEMM convolution launch of a sub-batch of an N-image run on
 * the current device with each tile shape that has a kernel instance (HIP events on `stream`) and keeps the fastest; a
 * tile only replaces the planner's choice for a > 3 % win.  Outputs are bit-identical for every tile.  Blocks until
 * done (tens of milliseconds); returns the number of launches whose tile changed, or a negative status. */
int f8_net_autotune(f8_net* net, int N, void* stream);

/* Pipelined submission (off by default).  By default a run starts after everything enqueued on `stream` before it,
 * which includes the PREVIOUS run's join: consecutive runs execute back to back.  With pipelining on, the caller
 * promises one call of slack on its buffers — the input of run i was complete, and the output buffer of run i free,
 * by the time run i-1 was submitted (static or double-buffered buffers) — and the sub-batches of run i then start as
 * soon as the sub-batches of run i-1 that use the same arena have finished: the tail of one run overlaps the head of
 * the next (its memory-bound early stages with the previous run's compute-bound late stages).  Results still become
 * visible in `stream` order (every run joins `stream`).  Same `stream` for consecutive pipelined runs.
 * on == 2: same contract, different schedule — every run executes UNSPLIT on one of two internal streams / arena copies,
 * alternating, so that two consecutive runs are in flight together: each launch covers the whole batch (twice the
 * workgroups of a sub-batch launch), which is what the latency-bound launches of the late stages need at 128 images;
 * the latency of one run roughly doubles, the throughput of a stream of runs rises. */
int f8_net_set_pipelined(f8_net* net, int on);

/* Orders the NEXT run (any f8_net_run* entry) behind `event` (a hipEvent_t passed as void*; NULL clears): the run's first
 * launch waits for it in addition to its stream dependencies.  This is how a pipelined caller hands over an input that is
 * produced on another stream (an H2D copy, a decoder): record the event behind the producer, call this, then run.  Needed
 * because under f8_net_set_pipelined the run does NOT wait for work queued on `stream` after the previous run's entry.
 * One-shot: consumed by the next run. */
int f8_net_set_input_ready(f8_net* net, void* event);

/* Device buffers of outputs 1 .. n of a net with more than one output: bufs_dev[k - 1] receives output k, NCHW [N,C,H,W],
 * int32 or float32 as its f8_net_output asked, as output_dev receives output 0.  n must be f8_net_num_outputs - 1
 * (F8_ERR_INVALID otherwise, and for a NULL buffer; a single-output net accepts n == 0 with any bufs_dev, which changes nothing).  One-shot, like f8_net_set_input_ready: the next run — any of f8_net_run,
 * _run_f32, _run_u8, _run_profiled — consumes the buffers, and a run of a multi-output net that was not given its buffers
 * returns F8_ERR_STATE without issuing anything.  Under f8_net_set_pipelined the caller's promise covers these buffers too:
 * one call of slack.  Option graph = 1: the replay key is (input, output, N, stream) and knows one output buffer, so a handle
 * with more than one output does not capture and runs plain launches. */
int f8_net_set_output_buffers(f8_net* net, void* const* bufs_dev, int n);

/* Blocks until the device is idle and reports failures that happened INSIDE kernels of earlier runs of this handle: the
 * stage-chain launches (option fuse_chain) exchange halo rows between workgroups and bound every wait (chain_timeout_ms); a
 * workgroup whose neighbour never arrives stores (run tag << 8 | code) in an error word, the launch runs on without waiting, and THAT run's
 * outputs are invalid — they are POISONED where they leave the library (the classifier / output kernel writes NaN, or INT32_MIN for int32
 * outputs, when the word carries its run's tag), so a caller that never calls this function cannot mistake them for results; later runs are
 * refused by f8_net_run until this function has been called.  F8_OK, or F8_ERR_HIP with the code in f8_last_error — the words of EVERY
 * arena copy are then cleared and the launches' ticket / flag words re-armed from the host (the device is idle).  It also reports (F8_ERR_INVALID) an int32 network input that held
 * values outside the head's 8-bit format in a run since the last check: f8_net_run NARROWS such an input to 8 bits where the reference
 * would feed the full int32 to the head conv (fix_train.py:689 only asserts >= 0), so out-of-format values cannot be honoured; the range
 * is checked inside the input / stem kernel (option check_input_range, default 1).  Never needed for correctness of a healthy run. */
int f8_net_check(f8_net* net);

/* Per-handle tuning options.  A new handle takes its defaults from the environment (F8_<KEY IN CAPITALS>; F8_CHUNK for
 * chunk56) and otherwise the measured best; two handles in one process may differ.  Keys that decide the plan must be set
 * before f8_net_finalize (F8_ERR_STATE afterwards); scheduling keys may change between runs.
 *   planning  : split (1..4 concurrent sub-batches of a run), arena_copies (0 = split; more: that many whole runs in flight under
 *               f8_net_set_pipelined(2) with pipeline_depth), fuse_blocks, fuse_stages (bit mask, -1 = auto), fuse_dual,
 *               fuse_ds, fuse_opener, fuse_fc (the classifier writes the caller's logits buffer itself), fuse_stem, fuse_input (the fused stem launch reads the caller's NCHW buffer itself), fuse_ir (1 = where it wins, 2 = every block), fuse_irk (off by default; 1: an inverted residual around a depthwise 5x5 or 7x7 — stride-1 1x1 expand, depthwise / 1 or 2 with pad = kernel / 2, stride-1 1x1 project, optionally joined with the block input at stride 1; block input of at most 192 and output of at most 320 padded channels, intermediates read by nobody else and no output — in ONE launch, the expanded tensors only in LDS, f8_irk.hip; everything else, pad < kernel / 2 included, stays three launches, and 3x3 blocks stay fuse_ir's; integer requantisation whatever requant_float says), fuse_irchain (off by default; 1: runs of >= 2 consecutive stride-1 MobileNet-V2 inverted residuals on a map of at most 256 pixels — the 14x14 and 7x7 runs at 224x224 — in ONE launch, one workgroup per image, nothing between the blocks in HBM, f8_irchain.hip), fuse_dws (off by default; 1: a MobileNet-V1 depthwise-separable block — depthwise 3x3 / 1 or 2, ReLU, 1x1 — whose output map is at least 28 or exactly 14 wide and whose readers all take int8 in ONE launch, the depthwise result only in LDS, f8_dws.hip; the blocks on 7-wide maps stay two launches: the matrix-core depthwise walker has no 7-wide form — see fuse_dws7), fuse_dws7 (off by default, independent of fuse_dws; 1: such a block whose OUTPUT map is exactly 7x7 — input 7x7 at stride 1 or 14x14 at stride 2 — in ONE launch, f8_dws7.hip: the depthwise conv on v_dot4, up to four images per workgroup, the output-channel tiles cut into slices over workgroups; where the block output's only reader is the average pool and the pooled tensor is not the network output the pool is summed in that launch and the block output never exists), fuse_head_dws (off by default; 1: the MobileNet-V1 head — network input -> 3x3 / 2 conv to 32 channels, ReLU -> depthwise 3x3 / 1, ReLU -> 1x1 to at most 64 channels, with or without ReLU, int8 readers in at most two formats, input sides multiples of 4, at most 224 wide — in ONE row-walking launch that reads the caller's buffer itself, f8_head_dws.hip; with fuse_dws the first depthwise-separable block belongs to this launch), fuse_chain (all consecutive bottleneck blocks of a stage in one launch, the int32 residual stream in registers; it takes precedence over fuse_stages and over the chunk56 / chunk28 / chunk14 keys for the stages it plans: set fuse_chain = 0 to get the per-block launches those keys govern), chain_stack (1: a 14x14 stage chain tiles image PAIRS as one 28-row map — 7 tiles of 4 rows per pair instead of 4 per image, zeros across the seam in the 3x3; same kernel symbol, 0: one image per tile column), fuse_tail (the join of a stride-2 stage-opening block opens that launch: its int32 output never exists), fuse_chain7 (the 7x7 bottleneck stage — that join, its identity blocks and the average pool behind them — as one launch over clusters of eight workgroups, f8_cchain.hip; 0: the dual-GEMM / fused_p12 / residual-join launches of rounds 3 - 5), fuse_pool (the network's last 1x1 conv, with its residual join, and the average pool behind it in one launch),
 *               fuse_bchain (the same for BasicBlock stages: 1 = consecutive identity blocks, 2 = with the stage-opening block in front), fuse_bchain7 (off by
 *               default; the 7x7 x 512 BasicBlock stage of ResNet-18 / 34 over clusters of eight workgroups, f8_bcchain.hip: 1 = its consecutive identity blocks
 *               in one launch, 2 = with the JOIN of the stage-opening block in front — its stride-2 body.0 stays a launch of its own; an average pool that
 *               is the stage output's only reader is summed in the same launch; requant_float = 1 plans run its integer instance), stem_rows (ResNet head:
 *               row-walking kernel, pool in registers), fuse_head2 (MobileNet-V2: head conv + depthwise + 1x1 as one row-walking launch), dw_mma (depthwise
 *               3x3 on the matrix cores), shared_streams (internal streams are one set per device for all handles), fuse_p12 (7x7 block: first two
 *               convs in one launch), wstat (weight-stationary 1x1 kernel: plain, dual-GEMM and residual-join instances) with
 *               wstat_min_tiles (pixel tiles per workgroup a launch must offer; 0 = always) and wstat_fast (0 = general epilogue), wreg (weights-streamed 1x1 kernel for the
 *               512 -> 256 / 1024 -> 512 reductions of smaller launches),
 *               patch3x3, dual_wide, deep_nk, bk128, igemm_tile (default 0; tests and tuning: 1 .. 4 force f8::conv_igemm_kernel's tile to 128x128 / 128x64 /
 *               64x128 / 64x64 where f8_net_autotune would try it — no 128-wide tile over at most 64 padded output channels, the dual-GEMM pair on
 *               64-wide tiles or 128x128, never 64x32; the K step stays.  0 changes nothing.  Same values with every tile), dw_dot4, dwk_dot4 (default 1; depthwise convs other than 3x3 / pad 1 — kernel 3 / 5 / 7, stride 1 / 2,
 *               pad 0 .. kernel / 2 —, always a launch of their own: 1 = a launch that writes int8 forms only runs f8::dwconvk_dot4_kernel<K, S>, f8_dwk.hip;
 *               0 = f8::dwconvk_kernel, which a launch that writes an int32 form runs either way.  dw_mma and dw_dot4 govern 3x3 / pad 1 only), opener_stg, whole_batch_launches (hint: runs will use
 *               f8_net_set_pipelined(2)),
 *               requant_float (default 0: INTEGER shift / round-half-even / clamp in every kernel — fix_quant_ops.py:99-112 literally, on gfx950's
 *               v_ashr_pk_u8_i32; no float instruction in any epilogue; 1: a ReLU -> unsigned-8-bit right shift (1..16) of a value the PLANNER
 *               CAN BOUND — conv accumulators, the int32 stream of a chain launch — runs through the float converter: v_cvt_f32_i32, v_mul_f32
 *               by 2^-n, v_cvt_pk_u8_f32: exact, compared with the reference's arithmetic over all 2^32 inputs on the device; anything
 *               unbounded takes the integer form by itself.  Same results either way, bit for bit.  The general depthwise launches
 *               (dwk_dot4) requantise in the integer form whatever this says: same kernels, same values),
 *               tap_tiled (default 1: the copy-out launches of outputs 1 .. run f8::tap_kernel, f8_tap.hip — one wave per 4 KB block of the
 *               int32 source, every loaded byte used; 0: f8::output_kernel, which walks the destination.  Output 0 always leaves through
 *               output_kernel or the classifier itself.  Same values either way),
 *               grouped (default 0: f8_net_conv refuses 1 < groups < cin with F8_ERR_UNSUPPORTED; 1: accepted — kernel 3, stride 1 / 2,
 *               pad 0 / 1, cin == cout, cin / groups in {2, 4, 8, 16, 32} run f8::gconv3x3_kernel, f8_gconv.hip, plan token gconv3x3s{S}:,
 *               every other grouped conv runs as the DENSE EXPANSION, the plain conv kernels over block-diagonal weights, plan token
 *               gconv{k}x{k}s{S}_dense:; 2: accepted, always the dense expansion.  Set it before the f8_net_conv call that adds the
 *               grouped conv.  Same values in both, bit for bit; depthwise convs keep their own rules and kernels whatever it says),
 *               concat_i8 (default 1: a concat whose result is read in at most two int8 formats and by nothing else, with values the planner can
 *               bound, runs f8::concat_i8_kernel on its operands' int8 forms, plan token concat_i8:; 0: every concat runs f8::concat_i32_kernel on
 *               their int32 forms, token concat_i32:.  Same values either way, bit for bit),
 *               upsample_i8 (default 1: a nearest upsample whose result is read in at most two int8 formats and by nothing else runs
 *               f8::upsample_i8_kernel on its source's int8 forms, plan token upsample_nearest_i8:; 0: it runs f8::upsample_i32_kernel<false> on the
 *               int32 form, token upsample_nearest_i32:.  Same values either way, bit for bit),
 *               sumpool_wide (default 1: a windowed average pool whose windows do not overlap (stride >= kernel) and whose kernel is at or above the
 *               measured crossover, 3, runs f8::sumpool_wide_kernel — a group of lanes per output value —, every other f8::sumpool_i32_kernel<K>;
 *               0: every pool runs the walker; 2: every pool with kernel >= 2 runs the wide kernel, for tests.  Same values on every leg, bit for bit),
 *               chanmap_i8 (default 1: a slice or channel shuffle whose result is read in at most two int8 formats and by nothing else moves bytes
 *               of its source's int8 forms, plan tokens slice_i8: / shuffle{g}_i8:; 0: every one runs f8::chanmap_i32_kernel on the int32 form, tokens
 *               slice_i32: / shuffle{g}_i32:.  Same values either way, bit for bit),
 *               fuse_shuffle (default 1: a concat of `groups` operands of one width that only an i8-mode shuffle reads emits no launch; the shuffle
 *               launch reads the operands, token concat+shuffle{g}_i8:; 0: two launches.  Same values either way, bit for bit),
 *               pixmap_i8 (default 1: a depth_to_space or space_to_depth whose result is read in at most two int8 formats and by nothing else moves
 *               bytes of its source's int8 forms, plan tokens d2s{r}{crd|dcr}_i8: / s2d{r}{crd|dcr}_i8:; 0: every one runs f8::pixmap_i32_kernel on the
 *               int32 form, tokens ..._i32:.  Same values either way, bit for bit),
 *               fuse_hgate (default 1: a hard gate whose only reader is the b operand of one f8_net_mul emits no launch; the mul launch reads the gate's
 *               source in int32, tokens hgate+mul_*: / hgate+chmul_*:; 0: an hgate: launch and the mul launch.  Same values either way, bit for bit),
 *               table_i8 (default 1: an f8_net_table whose result is read in at most two int8 formats and by nothing else gathers bytes from host-composed
 *               byte tables, token table_i8:; 0: every one runs the int32-mode kernel, token table_i32: — it reads the int32 entries and requantises on
 *               the device, and writes the int32 form only where something needs it.  Same values either way, bit for bit),
 *               fuse_table (default 1: a table whose only reader is the b operand of one broadcast f8_net_mul emits no launch where the map has fewer
 *               than 2^20 values an image — the measured rule, profiles/table_r15.md —, tokens table+chmul_*:; 2: on every size; 0: a table_*: launch
 *               and the mul launch.  Same values in every case, bit for bit),
 *               fuse_argmax (default 1: an f8_net_output_argmax on the result of an f8_net_upsample that nothing else reads is ONE launch that interpolates
 *               and reduces in registers, tokens upsample_bilinear+argmax_*: / upsample_nearest+argmax_*:, the upsampled tensor in no form; 0: the
 *               upsample launch and an argmax_*: launch.  Same class map either way, bit for bit)
 *   scheduling: chunk56 / chunk28 / chunk14 (images per chunk of the fused blocks; -1 = derived from chunk_budget_mb, 0 = whole
 *               batch), chunk_budget_mb (memory-side cache a chunk's int32 stream may occupy), chunk_ds, chunk_opener,
 *               split_streams, graph, stagger, stagger_pipelined, stem_wpc, stem_grid_div (row-walking head on 1 / n of the CUs; 0 = by output form), wstat_grid_div (0 .. 32, default 0, environment F8_WSTAT_GRID_DIV: f8::conv1x1_wstat_kernel sizes its pixel groups for 1 / n of the CUs, at least one — tests walk long tile rings on small maps; 0 = all of them; the plan and the values do not move), check_device, check_input_range, pipeline_depth (2..4 runs in flight),
 *               chain_timeout_ms (bound of a stage-chain launch's halo waits)
 *   read-only (f8_net_get_option): err_mirror (1 = after upload a page-locked host mirror of the chain error words exists: f8_net_run returns
 *               F8_ERR_HIP without issuing anything once a chain launch of an EARLIER run gave up waiting, until f8_net_check collects the error;
 *               0 = the mirror could not be allocated: time-outs surface only through f8_net_check / poisoned logits.  Multi-rank callers: a rank
 *               that is refused must still enter the step's collective — INTEGRATION.md "rank divergence")
 * F8_ERR_INVALID for an unknown key or a value outside the key's range. */
int f8_net_set_option(f8_net* net, const char* key, int value);
int f8_net_get_option(const f8_net* net, const char* key, int* value);

/* f8_net_run cuts a batch of N into this many independent sub-batches (1..4) that it runs on
 * internal streams forked from / joined to `stream` (no host synchronisation); every planned launch
 * is therefore issued this many times per run, each over N / parts images. */
int f8_net_num_parts(const f8_net* net, int N);

/* Kernel launches planned launch `i` issues in a run of N images under the current schedule: one per sub-batch, times the
 * chunks of images the launches that run chunked (the fused bottleneck blocks; F8_CHUNK*) are cut into.
 * f8_net_run_profiled reports the SUM over these launches for launch i. */
int f8_net_step_launches(const f8_net* net, int i, int N);

/* Same, bracketing every launch with HIP events on `stream`; ms[i] = duration of launch i summed over
 * the sub-batches, which run back to back on `stream` here (i < f8_net_num_launches).  Synchronises the stream before returning. */
int f8_net_run_profiled(f8_net* net, const int32_t* input_dev, void* output_dev, int N,
                        void* stream, float* ms, int cap);

/* Per-launch facts for roofline accounting: name (kernel + layer key), algorithmic bytes and
 * integer ops (2*MAC) for a batch of N.  Returns F8_ERR_INVALID if i is out of range. */
int f8_net_launch_info(const f8_net* net, int i, int N, char* name, size_t name_cap,
                       double* alg_bytes, double* alg_ops);

/* Device kernel symbol of launch i as rocprofv3 --kernel-trace prints it (without the argument list). */
/* ESSENTIAL vector lane-operations of planned launch i for N images: what the reference's element-wise semantics between the matrix products need in
 * their cheapest exact integer form — 3 per int8 value produced (int_op_only_fix_quant, fix_quant_ops.py:99-112: tie bit, rounding add, 1/2 shift-
 * saturate-pack, 1/4 merge, 1/4 bias flip), 2 per joined int32 value (fix_resnet.py:40-54: align-add + clamp / ReLU), 1 per max-pooled value.
 * The profile tooling divides the counters' vector instructions x 64 lanes by it (profiles/rocprof_*_valu.md: issued / essential). */
int f8_net_launch_valu(const f8_net* net, int i, int N, double* essential_lane_ops);
/* The device symbol (as rocprofv3 prints it) launch i starts.  Final once f8_net_finalize returns; only f8_net_autotune can still change it. */
int f8_net_launch_kernel(const f8_net* net, int i, char* buf, size_t cap);
/* Geometry of planned launch i when it is a stage chain, for N images on a device with num_cu compute units (0: 256): workgroups per tile
 * column, image groups (clusters) resident at once, grid, and images per tile column (2: image pairs, option chain_stack; 1 where the device
 * has too few compute units for a pair's tiles).  All four are 0 for other launches, and groups / grid are 0 where the device cannot run it. */
int f8_net_launch_grid(const f8_net* net, int i, int N, int num_cu, int* tiles, int* groups, int* grid, int* stack);

/* Attach a label (e.g. the state_dict key) to the node that produced tensor `t`. */
int f8_net_set_label(f8_net* net, int t, const char* label);

#ifdef __cplusplus
}
#endif
#endif /* F8NET_H */
