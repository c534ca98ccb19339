// f8_internal.h — kernel argument blocks and launchers shared by f8_kernels.hip and f8_net.cpp.
// Not part of the ABI (include/f8net.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace f8 {

// Per-handle tuning options (f8_net_set_option; include/f8net.h lists the keys).  Defaults are the measured best; the
// environment (F8_<KEY>) only seeds the defaults of a new handle, so two nets in one process can differ.
struct Options {
    int split = 2;               // concurrent sub-batches per run = arena copies (1..4)
    int fuse_blocks = 1;         // whole-bottleneck fusion
    int fuse_stages = -1;        // bit mask of stages for the identity-block fusion (-1: stages 0+1, stage 2 when a launch fills half the chip)
    int fuse_dual = 1;           // dual-GEMM downsample join
    int fuse_ds = 1;             // stage-opening block at unchanged resolution in one launch
    int fuse_opener = 1;         // stage-opening block with a stride-2 3x3 in one launch
    int fuse_fc = 1;             // the classifier writes the caller's logits buffer itself (no output launch)
    int fuse_stem = 1;           // stem conv + max-pool in one launch
    int fuse_input = 1;          // ... which also reads the raw network input (no input launch, no haloed NHWC4 copy)
    int wstat = 1;               // weight-stationary 1x1 kernel (f8_wstat.hip) where a launch gives every workgroup >= wstat_min_tiles pixel tiles
    int wstat_min_tiles = 2;
    int wstat_fast = 1;          // 0: always the general epilogue (requant in either direction, explicit ReLU floor)
    int wstat_grid_div = 0;      // tests: the weight-stationary 1x1 sizes its pixel groups for 1 / n of the CUs (long tile walks on small maps); 0 = all of them
    int s2wreg = 1;              // stride-2 3x3 convs of the stage-2 / stage-3 openers on conv3x3s2_wreg_kernel (f8_s2conv.hip)
    int wreg = 1;                // late 1x1 convs on conv1x1_wreg_kernel (weights straight to registers, f8_wreg.hip)
    int fuse_bchain = 2;         // consecutive BasicBlock identity blocks of a stage in ONE launch (f8_bchain.hip); 2: with the stage-opening block in front of them
    int fuse_bchain7 = 0;        // ... and those of a 7x7 x 512 stage over clusters of eight workgroups, the pool behind them summed in the launch (f8_bcchain.hip);
                                 // 2: with the JOIN of the stage-opening block in front of them (its stride-2 body.0 stays a launch of its own)
    int fuse_chain = 1;          // all consecutive bottleneck blocks of a stage in ONE launch, int32 residual stream in registers (f8_chain.hip)
                                 // with the same number of rounds (224): groups that finish a round early free their CUs for the next batch's launches
    int fuse_chain7 = 1;         // ... and the identity blocks of a 7x7 bottleneck stage over clusters of eight workgroups (f8_cchain.hip); 0: fused_p12 + the residual-carrying 1x1
    int fuse_pool = 1;           // the network's last 1x1 conv (+ residual join) and the average pool behind it in one launch (f8_pool.hip)
    int fuse_tail = 1;           // ... and the JOIN of a stride-2 stage-opening block as the first block of its stage's chain (its body.0 + body.2 on f8_opener.hip, P12)
    int chain_timeout_ms = 10000; // bound of its halo-exchange spins (another process holding the CUs for longer: sticky error word, logits poisoned, f8_net_check)
    int chain_stack = 1;         // stage chains whose H rows are not whole tiles but 2H are (14x14): image pairs as one 2H-row map, 7 tiles per pair instead of 8
    int fuse_p12 = 1;            // 7x7 identity blocks: body.0 + body.2 in one launch, split over a workgroup pair per image (f8_p12.hip)
    int fuse_head2 = 1;          // MobileNet-V2 head (3x3 / 2 conv, depthwise 3x3, 1x1) as one row-walking launch (f8_stem.hip, H2)
    int fuse_ir = 1;             // MobileNet-V2 inverted residual (expand -> depthwise -> project) in one launch: 1 = where it wins, 2 = always
    int fuse_irchain = 0;        // runs of >= 2 consecutive stride-1 inverted residuals on a small map in ONE launch, one workgroup per image (f8_irchain.hip)
    int fuse_irk = 0;            // inverted residual around a depthwise 5x5 / 7x7 (pad K / 2) in ONE launch (f8_irk.hip); K = 3 stays fuse_ir's
    int fuse_dws = 0;            // MobileNet-V1 depthwise-separable block (depthwise 3x3 -> 1x1) in ONE launch, the depthwise result only in LDS (f8_dws.hip)
    int fuse_head_dws = 0;       // MobileNet-V1 head + first depthwise-separable block (3x3 / 2 conv, depthwise 3x3, 1x1 to 32 / 64 channels [ReLU]) as one row-walking launch (f8_head_dws.hip)
    int fuse_dws7 = 0;           // ... the same for blocks whose OUTPUT map is 7 x 7, the average pool behind the last one summed in the launch (f8_dws7.hip)
    int patch3x3 = 1;            // LDS-patch 3x3 kernel
    int dual_wide = 2048;        // dual-GEMM joins with at least this many couts use the 128x128 tile
    int deep_nk = 7;             // K loops of at least this many steps use the deepest DMA ring
    int bk128 = 0;               // 128-byte K steps in conv_igemm_kernel
    int igemm_tile = 0;          // tests and tuning: 1 .. 4 force conv_igemm_kernel's tile to 128x128 / 128x64 / 64x128 / 64x64 where f8_net_autotune would try it (bk stays)
    int dw_dot4 = 1;             // v_dot4 depthwise kernel
    int dwk_dot4 = 1;            // general depthwise (not 3x3 / pad 1): the v_dot4 kernel of f8_dwk.hip for int8-only launches (0: its generic kernel)
    int dw_mma = 1;              // depthwise 3x3 on the matrix cores (f8_dwmma.hip) where it has an instance (output width >= 14, int8 outputs)
    int stem_rows = 1;           // ResNet head: the row-walking kernel (pool in registers) where it has an instance, else the tile kernel
    int stem_grid_div = 0;       // row-walking head on 1 / n of the CUs; 0 = all of them when it writes int32 (write-bound), half otherwise
    int stem_wpc = 3;            // resident stem workgroups per CU (2 / 3 / 4: 84.0 / 84.5 / 84.7 k img/s, same box)
    int opener_stg = 1;          // stride-2 opener: int8 output staged through LDS into 128-byte lines
    int chunk56 = -1, chunk28 = -1, chunk14 = -1;   // images per chunk of the fused blocks (-1: derived from chunk_budget_mb, 0: whole batch)
    int chunk_budget_mb = 96;    // a chunk's int32 stream must fit this much memory-side cache (3/8 of the 256 MiB Infinity Cache)
    int chunk_ds = 1, chunk_opener = 0;             // chunk the stage-opening blocks too (the stride-2 opener runs one workgroup per
                                                    // CU, 7 per image: measured 139 us in one 128-image launch, 161 us in 4 chunks)
    int whole_batch_launches = 0;   // planning hint: launches will cover the whole batch (f8_net_set_pipelined(2)), not max_batch / split images
    int pipeline_depth = 2;      // f8_net_set_pipelined(2): runs in flight (2..4, at most `split` arena copies)
    int shared_streams = 1;      // the internal streams are one set per device, shared by all handles (0: four streams of its own per handle)
    int arena_copies = 0;        // arena copies allocated at upload; 0 = `split`.  More than `split`: that many whole runs may be in flight
                                 // under pipelining mode 2 (pipeline_depth) while a non-pipelined run still cuts the batch `split` ways
    int split_streams = 1;       // 0: same launches serialised on the caller's stream (profiling)
    int graph = 0;               // hipGraph capture / replay of a run
    int stagger = -1, stagger_pipelined = 2;
    int check_device = 1;        // f8_net_run fails if the current device is not the one the handle was uploaded to
    int requant_float = 0;       // 0 (default since round 5: BASELINE north_star — no FP32 multiply in any epilogue): integer shift / round-half-even /
                                 // clamp in every kernel; 1: ReLU -> unsigned 8-bit right shifts of values the planner can bound may run through the
                                 // float converter (v_cvt_f32_i32, v_mul_f32 by 2^-n, v_cvt_pk_u8_f32: exact where planned, f8_device.h)
    int grouped = 0;             // grouped convs (1 < groups < cin): 0 = refused by f8_net_conv; 1 = accepted, on gconv3x3_kernel (f8_gconv.hip) where it applies and as the
                                 // dense expansion (the plain conv kernels over block-diagonal weights) elsewhere; 2 = accepted, always the dense expansion
    int concat_i8 = 1;           // f8_net_concat: 1 = the byte-gather mode where it is exact (every source written in the output's int8 formats, f8_concat.hip); 0 = always the int32 mode
    int upsample_i8 = 1;         // f8_net_upsample, nearest: 1 = the byte-copy mode where the result is read in at most two int8 formats and by nothing else (f8_upsample.hip); 0 = always the int32 mode
    int sumpool_wide = 1;        // f8_net_avgpool_window: 1 = sumpool_wide_kernel where sumpool_wide_rule says so (windows of 3 and more that do not overlap), else the block walker (f8_sumpool.hip);
                                 // 0 = every pool on the walker; 2 = every pool with kernel >= 2 on the wide kernel (tests).  Same values on every leg
    int chanmap_i8 = 1;          // f8_net_slice / f8_net_channel_shuffle: 1 = the byte-gather mode where the result is read in at most two int8 formats and by nothing else (f8_chanmap.hip); 0 = always the int32 mode
    int fuse_shuffle = 1;        // a concat read by one i8-mode channel shuffle alone, `groups` operands of one width: 1 = one launch that reads the concat's operands (concat+shuffle{g}_i8:); 0 = two launches
    int pixmap_i8 = 1;           // f8_net_depth_to_space / f8_net_space_to_depth: 1 = the byte-gather mode where the result is read in at most two int8 formats and by nothing else (f8_pixmap.hip); 0 = always the int32 mode
    int fuse_hgate = 1;          // a hard gate read by the b operand of one mul alone: 1 = no launch of its own, the mul launch reads the gate's int32 source (hgate+mul_*: / hgate+chmul_*:, f8_mul.hip); 0 = two launches
    int table_i8 = 1;            // f8_net_table: 1 = the byte-gather mode where the result is read in at most two int8 formats and by nothing else (table_i8:, f8_table.hip); 0 = always table_i32:
    int fuse_table = 1;          // a table read by the b operand of one broadcast mul alone: 1 = no launch of its own where the map has fewer than 2^20 values an image (the measured rule, fuse_table_rule in f8_net.cpp), the mul launch looks b up itself (table+chmul_*:, f8_table.hip); 2 = always; 0 = two launches
    int fuse_argmax = 1;         // an argmax output on an upsample's result that nothing else reads: 1 = one launch that interpolates and reduces in registers, the upsampled tensor in no form (upsample_*+argmax_*:, f8_argmax.hip); 0 = the upsample launch and an argmax_*: launch
    int tap_tiled = 1;           // network outputs 1 .. leave on tap_kernel (f8_tap.hip: walks the I32T blocks, every loaded byte used); 0: on output_kernel like output 0
    int check_input_range = 1;   // int32 inputs that are NARROWED to the head's 8-bit format (no requant) are range-checked on the device; f8_net_check reports
};
void options_from_env(Options* o);                       // f8_net.cpp
int* option_slot(Options* o, const char* key);            // nullptr: unknown key

// The largest right shift at which the float-converter requantisation is exact (requant_u8x4, f8_device.h)
constexpr int kRequantU8MaxShift = 16;

// One requantisation target format: int_op_only_fix_quant with n = src_fl - dst_fl.  Every Requant is made by of().
struct Requant {
    int32_t n;        // shift (> 0 right with round-half-even, <= 0 left)
    int32_t lo, hi;   // clamp bounds: [-127,127] or [0,255]
    uint32_t bias_xor; // 0x80808080 for unsigned formats (stored biased: x ^ 0x80), 0 for signed
    static Requant of(int n, bool sgn) { return sgn ? Requant{n, -127, 127, 0u} : Requant{n, 0, 255, 0x80808080u}; }
    // THE fast-instance rule: unsigned 8-bit by a right shift of 1 .. 30 — behind a ReLU (each *_inst / *_fast adds that and what else is its own)
    // this is what the FAST / FQ instances compute (requant_u8x4_int, f8_device.h).  Since of() is the only maker, lo == 0 alone (what the stage-chain
    // families used to test) and the full clamp / bias test are the same condition: every family states this one.
    __host__ __device__ bool u8_shr() const { return n > 0 && n <= 30 && lo == 0 && hi == 255 && bias_xor == 0x80808080u; }
    // ... and the float converter is exact for it: u8_shr() with the tighter bound, spelled out (one range test on the device)
    __host__ __device__ bool u8_float() const { return n > 0 && n <= kRequantU8MaxShift && lo == 0 && hi == 255 && bias_xor == 0x80808080u; }
};
// One requantised int8 output of an epilogue: a Requant with a pointer.  The pointer stands IN FRONT of the format, hence as a base of its own: that is the
// kernel-argument layout the stage-chain kernels were built with; behind the format, their SGPR spill counts and scratch sizes move.
struct QuantPtr { int8_t* ptr; };      // NHWC int8, row stride ld (bytes); nullptr = absent
struct QuantOut : QuantPtr, Requant {};

// A divisor known at finalize: n / d == (t + ((n - t) >> s1)) >> s2, t = high32(n * m); exact for every 32-bit n (Granlund-Montgomery round-up
// method, branch-free form).  Device side: fast_div (f8_device.h).
struct FastDiv { uint32_t m; int32_t s1, s2; };
inline FastDiv fast_divisor(uint32_t d) {                 // d >= 1
    int l = 0;
    while ((1ull << l) < d) ++l;                       // l = ceil(log2 d)
    return {(uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1), l < 1 ? l : 1, l > 1 ? l - 1 : 0};
}

// Implicit-GEMM int8 convolution / linear on v_mfma_i32_32x32x32_i8.
//   D[cout][pixel] = sum_k W[cout][k] * (X[pixel][k] ^ xor_mask)   (+ offset-corrected bias)
// X rows are gathered from an NHWC int8 tensor: K runs over taps (r,s) then CK bytes per tap.
struct ConvArgs {
    const int8_t* x;  uint32_t x_bytes;
    const int8_t* w;  uint32_t w_bytes;    // packed [coutP][ktot], K-contiguous
    const int32_t* bias;                   // [ncls][coutP] border-class bias table (see pack_conv_weights)
    const uint8_t* rowcls; const uint8_t* colcls;   // class of output row p / col q; ncc = #col classes
    int32_t ncc;                           // 0: single class (no padding, or signed input)
    int32_t M;                             // N*P*Q output pixels
    int32_t PQ, Q;
    FastDiv dPQ, dQ;                       // m / PQ and rem / Q
    int32_t sN, sP, sQ;                    // input byte strides: per image, per output row, per output col
    int32_t origin;                        // byte offset of tap (0,0) at p=q=0 (negative with padding)
    int32_t H, W, stride, pad, kh, kw;
    int32_t CK;                            // bytes per tap (multiple of BK)
    int32_t tapH, tapW;                    // byte offset per tap row / col
    int32_t ktot;                          // kh*kw*CK
    int32_t coutP;                         // padded cout = row stride of NHWC outputs (elements)
    // epilogue
    int32_t relu0;                         // ReLU directly after the conv
    const int32_t* res;                    // int32 NHWC residual operand or nullptr
    int32_t acc_shl, res_shl;              // alignment shifts (one of them is 0)
    int32_t relu1;                         // ReLU after the residual add
    int32_t* out32;                        // NHWC int32 (stride coutP) or nullptr
    QuantOut q[2];
    // dual GEMM (x2 != nullptr): a second 1x1 / pad 0 conv over the same output pixels whose result (+ bias2) is
    // the residual operand of the join; K steps of (x, w) run first, then those of (x2, w2)
    const int8_t* x2; uint32_t x2_bytes;
    const int8_t* w2; uint32_t w2_bytes;   // [coutP][ktot2]
    const int32_t* bias2;                  // [coutP]
    int32_t sN2, sP2, sQ2, ktot2;          // input byte strides of x2 (per image / output row / output col), its K
    void* trace;                           // tuning builds (F8_TRACE) only; nullptr otherwise
    int32_t dil, kwd;                      // conv_igemm_kernel only: dilation (1: none) and kw * dil — its K loop steps the tap coordinates by dil and wraps the column at kwd
    // conv_igemm_kernel only: the column axis of a rectangular conv (f8_net_conv_rect).  `stride` and `pad` are then the rows' stride and TOP pad, these the
    // columns' stride and LEFT pad; pad_far = the larger of the bottom / right pads, which no coordinate needs: it only decides, with the other two, whether
    // any tap can leave the image (padded()).  A square conv: stride_w = stride, pad_w = pad_far = pad.  The stem path: pad = pad_w = pad_far = 0.
    int32_t stride_w, pad_w, pad_far;
    bool padded() const { return pad > 0 || pad_w > 0 || pad_far > 0; }
};

// Depthwise K x K (groups == C), NHWC int8 in, VALU.  3x3 / pad 1: the launchers of f8_kernels.hip / f8_dwmma.hip, which never read `k`;
// every other accepted geometry (k 3 / 5 / 7, pad <= k / 2; k 3 at dilation dil > 1, pad <= dil: "general depthwise"): f8_dwk.hip, with the images of pack_dwk_weights.
struct DwArgs {
    const int8_t* x; const int8_t* w;      // w: [k * k][Cs] tap-major
    const int32_t* bias;                   // [Cs]
    const int8_t* w4; const int32_t* bias4; // dot4 kernels, bias + 128*sum(w) for unsigned inputs.  3x3 / pad 1: [Cs/4][9] tap-transposed dwords;
                                           // general: [Cs/4][k columns][ceil(k / 4) row groups][4 channels] dwords, byte j = row 4g + j (0 beyond k)
                                           // a strip (kw != k): [Cs/4][4 phases][ceil((k + 3) / 4)][4 channels] dwords, the taps shifted by `phase` bytes
    int32_t N, H, W, P, Q, Cs, stride, pad;
    int32_t in_signed;
    int32_t relu0;
    int32_t* out32;
    QuantOut q[2];
    int32_t band;                          // f8_dwmma.hip: output rows per wave (set by its launcher)
    int32_t acc_ok;                        // every accumulator is provably below 2^31 - 2^16 in magnitude (planner: conv_acc_bounded): the
                                           // float requantisation (requant_u8x4, f8_device.h) equals the wrapping integer one
    int32_t rq_int;                        // Options::requant_float == 0: integer requantisation only
    int32_t k;                             // kernel size; read by the general depthwise kernels only (f8_dwk.hip)
    int32_t dil;                           // ... and the dilation (1: none; > 1 only with k == 3)
    int32_t kw, pad_w;                     // ... and the columns' kernel size and leading pad: k and pad are the rows' (kernel height, top pad).  A square conv:
                                           // kw = k, pad_w = pad; a strip (f8_net_conv_rect): one of k / kw is 1.  The 3x3 launchers never read them.
};

// Grouped 3x3 (f8_gconv.hip): cin == cout, cg = C / groups divides 32, stride 1 / 2, pad 0 / 1.  The kernel sees 32-channel slices only.
struct GConvArgs {
    const int8_t* x; uint32_t x_bytes;     // NHWC int8 [N][H][W][Cs]
    const int8_t* w;                       // [Cs / 32 slices][9 taps][64 lanes][16 B]: block-diagonal 32 x 32 tap blocks in MFMA-fragment order (pack_gconv_weights)
    const int32_t* bias;                   // [ncls][Cs] border-class bias table (as ConvArgs)
    const uint8_t* rowcls; const uint8_t* colcls; int32_t ncc;   // class of output row p / col q; ncc = 0: single class
    int32_t N, H, W, P, Q, Cs, stride, pad;
    int32_t R, TW, G;                      // a workgroup's tile: R output rows x TW output columns of G images (gconv_tile; G > 1: whole images)
    int32_t tiles_r, tiles_c;              // tiles per image
    int32_t PR, PW;                        // its haloed input patch, pixels per image: (R - 1) stride + 3 rows of (TW - 1) stride + 3
    FastDiv dIPP, dPW, dRTW, dTW;          // / (PR * PW), / PW, / (R * TW), / TW
    int32_t relu0;
    int32_t* out32;
    QuantOut q[2];
};

struct PoolArgs {                          // max-pool, NHWC
    const void* x; int32_t in_is_i8, in_signed;
    int32_t N, H, W, P, Q, Cs, k, stride, pad;
    int32_t* out32;
    QuantOut q[2];                         // when in_is_i8: q[0].ptr is the int8 output, no requant
};

struct AvgArgs {                           // FXQAvgPool2d sum over H*W, NHWC int32 in
    const int32_t* x; int32_t N, HW, Cs;
    int32_t* out32;                        // [N][Cs] or nullptr
    QuantOut q[2];
};

struct AddArgs {                           // standalone align-add (when it cannot be fused) / requant
    const int32_t* a; const int32_t* b; int32_t M, Cs;   // M pixels x Cs channels, int32 in I32T layout
    int32_t a_shl, b_shl, relu;
    int32_t* out32;
    QuantOut q[2];
};

struct InArgs {                            // network input: int32 NCHW -> NHWC forms
    const int32_t* x; int32_t N, C, H, W;
    const float* xf; float scale; int32_t qlo, qhi;   // fp32 images quantised on the fly (x unused): rint(xf * scale) clamped
    const uint8_t* xu8; int32_t u8_nhwc;              // uint8 images (f8_net_run_u8): NCHW planes or NHWC pixels, through `lut`
    int16_t lut[3 * 256];                             // lut[c * 256 + byte] = the head-format integer of that pixel value
    uint32_t xor8;                         // 0x80808080 when the int8 consumer format is unsigned (biased storage)
    uint32_t* err; int32_t chk_lo, chk_hi; // err != nullptr: int32 inputs narrowed to 8 bits are checked against [chk_lo, chk_hi] (sticky error word)
    int8_t* out8;  int32_t Cs8;            // NHWC int8 (Cs8-channel rows), or
    int8_t* stem;  int32_t Hp, Wp, pad;    // zero-haloed NHWC4 for the stem conv
    int32_t* out32; int32_t Cs32;
};

// Channel concatenation (f8_concat.hip; f8_net_concat): K sources of one map side by side along C.  Mode i8 (concat_i8_kernel): src[k][i] is source i
// in the int8 format of output form k (NHWC, Cs_src[i]-byte rows), the launch copies bytes and only q[k].ptr / bias_xor are read.  Mode i32
// (concat_i32_kernel): src[0][i] is source i's int32 form (I32T), shifted left by shl[i] (wrapping), clamped to +-(2^31 - 1); out32 and q[] as AddArgs.
constexpr int kMaxConcat = 8;              // = F8_MAX_CONCAT (include/f8net.h)
struct ConcatArgs {
    const void* src[2][kMaxConcat];
    int32_t C[kMaxConcat], Cs_src[kMaxConcat], off[kMaxConcat], shl[kMaxConcat];   // real / padded channels of source i, its first output channel, its alignment shift
    int32_t K, M, Cs;                      // sources, pixels N * H * W, padded output channels (the real ones: off[K - 1] + C[K - 1])
    int32_t* out32;
    QuantOut q[2];
};

// Upsampling (f8_upsample.hip; f8_net_upsample): [C, Hs, Ws] -> [C, P, Q] = [C, Hs * sh, Ws * sw].  Mode i8 (upsample_i8_kernel, nearest only): src[k] is the
// source in the int8 format of output form k (NHWC, Cs-byte rows), the launch copies bytes and only q[k].ptr is read.  Mode i32 (upsample_i32_kernel):
// src[0] is the source's int32 form (I32T); nearest copies, bilinear (sh == sw == 1 << k) sums the four clamped neighbours with the integer weights of
// f8net.h (the exact value times 4 s^2, wrapping); out32 and q[] as AddArgs.
struct UpsampleArgs {
    const void* src[2];
    int32_t N, C, Cs, Hs, Ws, P, Q, sh, sw, k;           // images, real / padded channels, source map, output map, scales, bilinear: log2 of the scale
    FastDiv dPQ, dQ, dSh, dSw, dWs, dVpp;                // / (P * Q), / Q, / sh, / sw, / Ws, / (Cs / 16)
    int32_t* out32;
    QuantOut q[2];
};

// Windowed average pooling (f8_sumpool.hip; f8_net_avgpool_window): [C, H, W] -> [C, P, Q], each output the wrapping int32 sum of its k x k window's
// in-image taps.  x is the source's int32 form (I32T); out32 and q[] as AddArgs.
struct SumPoolArgs {
    const int32_t* x;
    int32_t N, C, Cs, H, W, P, Q, k, stride, pad;        // images, real / padded channels, source map, output map, window
    int32_t lg;                                          // sumpool_wide_kernel: log2 of the lanes that share one (output pixel, 4 channels) item (sumpool_wide_lg)
    FastDiv dPQ, dQ, dK, dCg;                            // / (P * Q), / Q, / k, / (Cs / 4)
    int32_t* out32;
    QuantOut q[2];
};
// The walker / wide rule of option sumpool_wide = 1, MEASURED (profiles/sumpool_r12.md, tools/ab_avgpool.py): windows that do not overlap (stride >= kernel)
// of this size and more run sumpool_wide_kernel — at 3x3 / 3 it takes 0.82 of the walker's time, at 4x4 / 4 0.38, at 2x2 / 2 1.3 - 2.1.  Overlapping
// windows (stride < kernel) stay on the walker, whose neighbouring lanes share their taps through the cache: measured up to 7x7 / 1 (the wide kernel
// 1.3 - 2.0 x its time); NOT measured above 7.
constexpr int kSumpoolWideKernel = 3;
inline bool sumpool_wide_rule(int kernel, int stride) { return kernel >= kSumpoolWideKernel && stride >= kernel; }

// Channel slice and channel shuffle (f8_chanmap.hip; f8_net_slice, f8_net_channel_shuffle): pure channel gathers of one map, out[c] = src[first + c]
// (groups == 0) or out[c] = src[(c % groups) * Cg + c / groups], Cg = C / groups.  The source is a TABLE of K entries: a slice has one (offset
// `first`); a shuffle has one per group — stand-alone every entry points at the source with offset i * Cg, fused with its concat (concat+shuffle)
// entry i is concat operand i with offset 0: the launches differ in nothing else.  Mode i8: src[k][i] is entry i in the int8 format of output form k
// (NHWC, Cs_src[i]-byte rows), the launch moves bytes and only q[k].ptr / bias_xor are read.  Mode i32 (chanmap_i32_kernel, never fused): src[0][0] is the
// source's int32 form (I32T); out32 and q[] as AddArgs.
struct ChanMapArgs {
    const void* src[2][kMaxConcat];
    int32_t Cs_src[kMaxConcat], off[kMaxConcat];         // row stride (padded channels) of entry i, its first channel
    int32_t K, groups, Cg;                               // table entries; 0 = slice, else the shuffle's groups (== K) and channels per group
    int32_t M, C, Cs;                                    // pixels N * H * W, real / padded output channels
    FastDiv dG;                                          // / groups
    int32_t* out32;
    QuantOut q[2];
};

// Depth-to-space and space-to-depth (f8_pixmap.hip; f8_net_depth_to_space, f8_net_space_to_depth): pure gathers between the channel axis and r x r
// pixel blocks of one map, the formulas of include/f8net.h.  (C, Cs, P, Q) are the OUTPUT's real / padded channels and map, (Csrc, Cs_src, Hs, Ws) the
// source's: s2d == 0: Csrc == C r^2, P == Hs r, Q == Ws r; s2d == 1: C == Csrc r^2, Hs == P r, Ws == Q r.  Mode i8: src[k] is the source in the int8
// format of output form k (NHWC, Cs_src-byte rows), the launch moves bytes and only q[k].ptr / bias_xor are read.  Mode i32 (pixmap_i32_kernel): src[0]
// is the source's int32 form (I32T); out32 and q[] as AddArgs.
struct PixMapArgs {
    const void* src[2];
    int32_t N, C, Cs, P, Q;                              // images, the output's real / padded channels and map
    int32_t Csrc, Cs_src, Hs, Ws;                        // the source's real / padded channels and map
    int32_t r, s2d, crd;                                 // block; 0 = depth_to_space, 1 = space_to_depth; 0 = F8_ORDER_DCR, 1 = F8_ORDER_CRD
    FastDiv dPQ, dQ, dHsWs, dWs, dR, dRR, dC;            // / (P * Q), / Q, / (Hs * Ws), / Ws, / r, / r^2, / Csrc (space_to_depth in DCR order: channel -> block)
    int32_t* out32;
    QuantOut q[2];
};

// Fixed-point multiply and hard gate (f8_mul.hip; f8_net_mul, f8_net_hard_gate).  out = A * B per element (bcast == 0: b has a's shape) or
// out[pixel m][c] = A[m][c] * B[image m / HW][c] (bcast == 1: b is [C, 1, 1]); `a` is operand a in the int8 format ra (NHWC, Cs-byte rows; the shift
// of ra is the producer's business: only ra.bias_xor and the sign ra.lo < 0 are read).  gate == 0: `b` is operand b in the int8 format rb, likewise.
// gate == 1 (a hard gate fused into the launch): `b` is the GATE's SOURCE in int32 (I32T; bcast: one pixel per image), the launch computes
// clamp(x, -lim, lim) + lim and requantises it by rb (shift, clamp) itself.  relu: max(., 0) on the product.  out32 (I32T) and q[] as AddArgs.
// The stand-alone hard gate (hgate_kernel) uses the same record: `b` is its int32 source, lim its 3 * 2^fl, a is unused.
struct MulArgs {
    const int8_t* a; const void* b;
    int32_t M, C, Cs;                                    // pixels N * H * W, real / padded channels (b's rows have the same Cs)
    int32_t HW; FastDiv dHW;                             // bcast: pixels per image, pixel -> image
    FastDiv dVpp;                                        // mul_i8_kernel: / (Cs / V), the vectors of a pixel (V = mul_vector_bytes of the instance)
    int32_t bcast, gate, relu;
    int32_t lim;                                         // gate: 3 * 2^fl of the gate's source
    Requant ra, rb;                                      // the operand formats (Requant::of)
    int32_t* out32;
    QuantOut q[2];
};

// The 256-entry table op (f8_table.hip; f8_net_table).  `src` is the source in the int8 format the table is indexed in (NHWC, Cs-byte rows, written
// by the source's producer); the stored byte ^ 0x80 is the index u for either sign of that format (unsigned: u = q; signed: u = q + 128).
//   table_i8_kernel     out form k byte = bt[k][u]: 256 bytes per output form, composed on the host (entry requantised to the form, storage bias folded in)
//   table_i32_kernel    out = t32[u] (the caller's 256 entries), written as int32 (I32T) and requantised to q[] as AddArgs
// Pad channels [C, Cs) of every output are the format's zero whatever the source's pad bytes hold.
struct TableArgs {
    const int8_t* src;
    int32_t M, C, Cs;                                    // pixels N * H * W, real / padded channels (source and result alike)
    FastDiv dVpp;                                        // table_i8_kernel: / (Cs / V), the vectors of a pixel
    const int32_t* t32;                                  // table_i32_kernel: the entries
    const uint8_t* bt[2];                                // table_i8_kernel: the composed byte table of q[k]
    int32_t* out32;
    QuantOut q[2];
};
// A table fused into the broadcast mul that reads it (table_chmul_*_kernel, f8_table.hip): m is the mul's record with gate == 0, bcast == 1 and
// m.b = the TABLE's source in its int8 index format (N rows of Cs bytes); bt is the byte table composed for the mul's format of b (m.rb).
struct TableMulArgs { MulArgs m; const uint8_t* bt; };

// Transposed convolution (f8_deconv.hip; f8_net_conv_transpose), stride 2 .. 4: [H, W] -> [P, Q] = [(H - 1) s - 2 pad + k + output_padding, ...].  The output
// pixels of one PHASE (rh, rw) = ((oh + pad) % s, (ow + pad) % s) see the same kernel taps kh = rh + s th, th < Th, at the input rows ih = a - th
// (oh = s a + rh - pad): one phase is one plain implicit GEMM over its sub-grid of A x Cn output pixels per image, K = Th * Tw * CK.
constexpr int kMaxDeconvPhases = 16;       // stride <= 4
struct DeconvPhase {
    int32_t rh, rw;                        // the phase
    int32_t a0, c0, A, Cn;                 // first row / column index (a, c) of its sub-grid, the sub-grid's rows / columns (0: the phase has no output pixel)
    int32_t Th, Tw;                        // live taps per axis: ceil((k - rh) / s), ceil((k - rw) / s); 0: its outputs are the bias alone
    uint32_t w_off;                        // byte offset of its packed weights [coutP][Th * Tw * CK] in MFMA-fragment order: [cout tile][K32 step][lane][16 B] (pack_deconv_weights)
    FastDiv dAC, dC;                       // / (A * Cn), / Cn
};
struct DeconvArgs {
    const int8_t* x; uint32_t x_bytes;     // NHWC int8 [N][H][W][CK]
    const int8_t* w; uint32_t w_bytes;     // the phases' weight matrices, one behind the other
    const int32_t* bias;                   // [row classes * ncc][coutP] border-class bias table; ncc = 0: one class
    const uint8_t* rowcls; const uint8_t* colcls; int32_t ncc;   // class of OUTPUT row oh / column ow: the set of kernel rows that meet an in-image input row
    int32_t N, H, W, P, Q, CK, coutP, stride, pad, nph;
    int32_t relu0;
    int32_t* out32;
    QuantOut q[2];
    int32_t tiles;                         // pixel tiles (64 pixels: a wave's two MFMA tiles) of the largest phase at N images (set by the launcher)
    DeconvPhase ph[kMaxDeconvPhases];
};

struct OutArgs {                           // NHWC int32 -> NCHW int32 / float32
    const int32_t* x; int32_t N, C, HW, Cs;
    void* out; int32_t as_float;
    const uint32_t* err; uint32_t epoch;   // the run's stage-chain error word (or nullptr) and tag: when the word carries THIS run's tag, the outputs are poisoned (NaN / INT32_MIN)
};

// Channel argmax as a network output (f8_argmax.hip; f8_net_output_argmax): out[n, p, q] = the smallest c with the largest x[n, c, p, q], uint8 or int32
// [N, P, Q] in the caller's buffer.  argmax_i32t_kernel: x is the marked tensor's int32 form (I32T), [C, P, Q]; only N, C, Cs, P, Q are read.
// upsample_argmax_kernel (option fuse_argmax): x is the int32 form of the SOURCE [C, Hs, Ws] of the upsample that produces the marked tensor, which
// exists in no form; scales, k and the divisors as UpsampleArgs.
struct ArgmaxArgs {
    const int32_t* x;
    int32_t N, C, Cs, Hs, Ws, P, Q, sh, sw, k;           // images, real / padded channels, source map, output map, scales, bilinear: log2 of the scale
    FastDiv dSh, dSw, dQ4, dP;                           // / sh, / sw, / ceil(Q / 4), / P
    void* out;                                           // the caller's buffer from this sub-batch's first image on
    const uint32_t* err; uint32_t epoch;                 // as OutArgs: when the word carries THIS run's tag the map is poisoned (255 / INT32_MIN)
};

// One launch for a ResNet bottleneck identity block (f8_fused.hip).
struct FusedArgs {
    const int8_t* x8; uint32_t x_bytes;    // block input, int8 NHWC [N*H*W][C] in body.0's input format
    const int32_t* xr;                     // block input, int32 I32T (residual operand)
    const int8_t* w0; const int8_t* w2; const int8_t* w4; uint32_t w0_bytes, w2_bytes, w4_bytes;   // [MID][C], [MID][9][MID], [C][MID]
    const int32_t* b0; const int32_t* b2; const int32_t* b4;                                        // offset-corrected biases
    // DS variant (wsc != nullptr): the join's other operand is the shortcut conv Wsc[COUT][C] . x (+ bsc) instead of xr
    const int8_t* wsc; uint32_t wsc_bytes; const int32_t* bsc; int32_t COUT;
    int32_t N, H, W, C, MID, R, tiles_per_img;
    Requant r1;                            // requant body.0 output -> body.2 input format
    Requant r2;                            // requant body.2 output -> body.4 input format
    int32_t relu_a, relu_b;                // ReLU after body.0 / body.2
    int32_t acc_shl, res_shl, relu1;       // residual join
    int32_t* out32; QuantOut q[2];
    void* trace;                           // tuning builds (F8_TRACE) only
    int32_t stride2;                       // stage-opening block with a stride-2 3x3 (f8_opener.hip): H, W are the INPUT map
    int32_t acc_ok, rq_int;                // P12: both convs' accumulators bounded (conv_acc_bounded) / Options::requant_float == 0 (see DwArgs)
    int32_t p12only;                       // f8_opener.hip: body.0 + body.2 only, q[0] = body.2's output (NHWC int8, MID channels); the join runs as the
                                           // first block of the stage's chain launch (ChainArgs::tail)
};

// One launch for ALL consecutive bottleneck blocks of a ResNet stage (f8_chain.hip): the int32 residual stream of a tile stays in
// registers from block to block.  Weight pointers are the MFMA-fragment-order images (pack_frag_weights).
struct ChainBlk {
    const int8_t* w0; const int8_t* w2; const int8_t* w4; const int8_t* wsc;     // wsc / bsc: stage-opening block only (1x1 shortcut conv)
    const int32_t* b0; const int32_t* b2; const int32_t* b4; const int32_t* bsc;  // offset-corrected, single class
    Requant rq;                            // requant block input (int32 stream) -> body.0's input format
    Requant r1;                            // requant body.0 output -> body.2 input format
    Requant r2;                            // requant body.2 output -> body.4 input format
    int32_t relu_a, relu_b, relu1;         // ReLU after body.0 / body.2 / the join
    int32_t acc_shl, res_shl;              // residual join: (conv << acc_shl) + (other << res_shl)
};
// The stage-chain kernels' exchange scratch and error reporting (f8_chain_common.h holds the protocol that uses it)
struct ChainSync {
    uint32_t* sync;                        // [0] ticket, [1] workgroups out, [16 + workgroup] exchange flag; zeroed by the last workgroup out
    uint32_t* err;                         // error word (a wait timed out): (epoch << 8) | code; read by f8_net_check
    uint32_t* err_host;                    // the same word's mirror in host-visible (pinned, mapped) memory: f8_net_run reads it WITHOUT a synchronisation and
                                           // refuses further runs until f8_net_check has collected the error (nullptr: no mirror)
    uint32_t epoch;                        // this run's tag (1 .. 2^24 - 1): only an error of THIS run ends waits early / poisons the logits —
                                           // a word left by an earlier run stays for f8_net_check to report and changes nothing else
    int8_t* xchg;                          // exchanged data (f8_chain.hip: halo rows between vertically adjacent tiles, [workgroup][parity][side][W * MID])
    uint32_t timeout_ticks;                // bound of every wait (100 MHz wall clock)
};

constexpr int kChainMaxBlocks = 6;
struct ChainArgs {
    ChainBlk blk[kChainMaxBlocks]; int32_t nblk;
    int32_t acc_ok;                        // body.0 / body.2 accumulators of every block bounded (see DwArgs::acc_ok)
    int32_t stream_ok;                     // ... and so is the int32 stream after every block (and the stream a chain of identity blocks reads): f8_net.cpp tensor_amax
    int32_t rq_int;                        // Options::requant_float == 0: integer requantisation everywhere (no float-converter instance)

    const int32_t* xr;                     // first block an identity block: the stage's int32 stream (I32T) — its int8 form is computed in the launch
    const int8_t* x8in;                    // first block a stage-opening block: its int8 NHWC input [N*H*W][CIN0] in body.0's / the shortcut's format
    // tail != 0: the first block is only the JOIN of a stage-opening block with a stride-2 3x3 (body.0 + body.2 ran in f8_opener.hip, P12):
    // x8in = the block input at TWICE the resolution [N][2H][2W][CIN0] in the SHORTCUT's int8 format (its pixels (2p, 2q) are the 1x1 / 2
    // shortcut's operand), m2in = body.2's output [N*H*W][MID] in body.4's int8 input format; blk[0] carries wsc / bsc / w4 / b4 / the join
    const int8_t* m2in; int32_t tail;
    int32_t N, NG;                         // images; image groups resident at once (grid = NG * tiles per image)
    int32_t* out32; QuantOut q[2];         // forms of the last block's output
    ChainSync cs;
    void* trace;
    int32_t R;                             // rows per tile of the instance to launch (chain_shape)
    int32_t pool;                          // f8_cchain.hip only: out32 / q[] are forms of the AVERAGE POOL behind the last block ([N][C]: FXQAvgPool2d's wrapping int32 sum over the map)
    int32_t stack;                         // images per tile column: 2 = image pairs tiled as one 2H-row map (instances with H % R != 0 == 2H % R: chain_stackable); 0 / 1 = one image
};
constexpr int kChainSyncWords = 16 + 512;   // [0] ticket, [1] workgroups out, [16 + workgroup] halo flags (up to two workgroups per CU)
constexpr int kChainErrWord = 1000;          // the sticky error word, inside the first 4096 bytes of the scratch
constexpr size_t kChainXchgBytes = (size_t)512 * 2 * 2 * 3584;

// One launch for consecutive BasicBlock identity blocks of a ResNet-18 / 34 stage (f8_bchain.hip); weights in fragment order.
struct BChainBlk {
    const int8_t* wa; const int8_t* wb;    // first / second 3x3
    const int32_t* ba; const int32_t* bb;  // offset-corrected, single class (the LDS patches carry a biased-zero border)
    Requant rq;                            // requant block input (int32 stream) -> the first conv's input format
    Requant r1;                            // requant first conv output -> second conv's input format
    int32_t relu_a, relu1;                 // ReLU after the first conv / after the join
    int32_t acc_shl, res_shl;              // join: (conv << acc_shl) + (stream << res_shl)
};
constexpr int kBChainMaxBlocks = 6;
struct BChainArgs {
    BChainBlk blk[kBChainMaxBlocks]; int32_t nblk;
    int32_t acc_ok;                        // first-conv accumulators of every block bounded (see DwArgs::acc_ok)
    int32_t stream_ok;                     // ... and the int32 stream after every block / the stream an identity-block chain reads (see ChainArgs)
    int32_t rq_int;                        // Options::requant_float == 0 (see ChainArgs)

    const int32_t* xr;                     // the stage's int32 stream (I32T): chains of identity blocks
    // chains that start with the stage-opening block (blk[0]: wa = 3x3 / 2 over C/2 channels, wb = 3x3, the stream = its 1x1 / 2 shortcut):
    const int8_t* x8in;                    // int8 NHWC input [N][2H][2W][C/2] in the format blk[0].wa reads
    const int8_t* x8sc;                    // ... in the format the shortcut reads (may be the same buffer)
    const int8_t* wsc; const int32_t* bsc; // shortcut conv, fragment order / offset-corrected bias
    int32_t N, NG;
    int32_t* out32; QuantOut q[2];
    ChainSync cs;
    void* trace;
};

// One launch for consecutive BasicBlocks of a 7x7 x 512 stage over clusters of eight workgroups (f8_bcchain.hip; option fuse_bchain7).  Blocks as
// BChainArgs.  tail != 0: blk[0] is only the JOIN of the stage-opening block (its wb / bb = body.2, acc_shl / res_shl: (body.2 << acc_shl) +
// (shortcut << res_shl)); body.0 ran in an earlier launch.
struct BCChainArgs {
    BChainBlk blk[kBChainMaxBlocks]; int32_t nblk;
    const int32_t* xr;                     // identity first block: the stage's int32 stream (I32T)
    const int8_t* m0in;                    // tail: body.0's output [N*7*7][512] in body.2's int8 input format
    const int8_t* x8sc;                    // tail: the block input [N][14][14][256] in the shortcut's int8 format
    const int8_t* wsc; const int32_t* bsc; // tail: shortcut conv, fragment order / offset-corrected bias
    int32_t tail, pool;                    // pool: out32 / q[] are forms of the AVERAGE POOL behind the last block ([N][512], FXQAvgPool2d's wrapping sum)
    int32_t N, NG;                         // images; clusters resident at once (grid = 8 NG)
    int32_t* out32; QuantOut q[2];
    ChainSync cs;
};

// One launch for a MobileNet-V2 inverted-residual block: 1x1 expand -> depthwise 3x3 -> 1x1 project [+ int32 residual] (f8_ir.hip).
struct IRArgs {
    int32_t acc_ok;                        // expand / depthwise accumulators bounded (see DwArgs::acc_ok)
    int32_t rq_int;                        // Options::requant_float == 0: integer requantisation only
    const int8_t* x8;                      // block input, int8 NHWC [N*H*W][CIN_S] in the expand conv's input format
    const int32_t* xr;                     // block input, int32 I32T (residual operand) or nullptr
    const int8_t* w0; const int32_t* b0;   // expand  [E32][CIN_S], offset-corrected bias [E32]
    const int8_t* wd4; const int32_t* bd4; // depthwise: dot4 image [E32/4][36 B], bias (+128*sum(w) for unsigned inputs) [E32]
    const int8_t* w4; const int32_t* b4;   // project [COUT_S][E32], offset-corrected bias [COUT_S]
    int32_t N, H, W, Ho, Wo, stride, R, G, tiles_per_img, E32;
    // The two inner formats stay LOOSE fields here and in IRKArgs (r1() / r2() read them as records): as nested Requant members, whatever the kernels'
    // spelling, the SGPR spill count of one generic instance here and two of fused_irk_kernel moves (profiles/argrec_kernel_resources.md)
    int32_t n1, lo1, hi1; uint32_t xor1;   // requant expand output -> depthwise input format
    int32_t n2, lo2, hi2; uint32_t xor2;   // requant depthwise output -> project input format
    Requant r1() const { return {n1, lo1, hi1, xor1}; }
    Requant r2() const { return {n2, lo2, hi2, xor2}; }
    void set_r(const Requant& f1, const Requant& f2) { n1 = f1.n; lo1 = f1.lo; hi1 = f1.hi; xor1 = f1.bias_xor; n2 = f2.n; lo2 = f2.lo; hi2 = f2.hi; xor2 = f2.bias_xor; }
    int32_t relu_a, relu_b, relu0;         // ReLU after expand / depthwise / project
    int32_t acc_shl, res_shl, relu1;       // residual join
    int32_t* out32; QuantOut q[2];
    int32_t xp, off_patch, off_mid2, off_w;   // LDS layout (filled by launch_fused_ir)
    FastDiv dW, dHW, dWo, dRWo;            // / W, / (H*W), / Wo, / (R*Wo)
};

// One launch for an inverted-residual block around a depthwise K x K, K = 5 / 7, pad K / 2 (f8_irk.hip): IRArgs with run-time channel counts.
struct IRKArgs {
    const int8_t* x8;                      // block input, int8 NHWC [N*H*W][cin] in the expand conv's input format
    const int32_t* xr;                     // block input, int32 I32T (residual operand) or nullptr
    const int8_t* w0; const int32_t* b0;   // expand  [E32][cin], offset-corrected bias [E32]
    const int8_t* wd4; const int32_t* bd4; // depthwise: pack_dwk_weights' dot4 image [E32/4][K][ceil(K/4)][4] dwords, bias (+128*sum(w) for unsigned inputs) [E32]
    const int8_t* w4; const int32_t* b4;   // project [cout][E32], offset-corrected bias [cout]
    int32_t K, cin, cout;                  // depthwise kernel size; channel counts padded to 32
    int32_t N, H, W, Ho, Wo, stride, R, G, tiles_per_img, E32;   // R output rows per tile (tiles_per_img = ceil(Ho / R)) or G whole images (irk_config)
    int32_t n1, lo1, hi1; uint32_t xor1;   // requant expand output -> depthwise input format (xor1 is also the patch's pad value); loose: see IRArgs
    int32_t n2, lo2, hi2; uint32_t xor2;   // requant depthwise output -> project input format
    Requant r1() const { return {n1, lo1, hi1, xor1}; }
    Requant r2() const { return {n2, lo2, hi2, xor2}; }
    void set_r(const Requant& f1, const Requant& f2) { n1 = f1.n; lo1 = f1.lo; hi1 = f1.hi; xor1 = f1.bias_xor; n2 = f2.n; lo2 = f2.lo; hi2 = f2.hi; xor2 = f2.bias_xor; }
    int32_t relu_a, relu_b, relu0;         // ReLU after expand / depthwise / project
    int32_t acc_shl, res_shl, relu1;       // residual join
    int32_t* out32; QuantOut q[2];
    int32_t xp, off_patch, off_mid2, off_w;   // LDS layout (filled by launch_fused_irk)
    int32_t QS;                            // P2 items per output row: ceil(Wo / 4)
    FastDiv dW, dHW, dWo, dRWo, dQS, dRQS; // / W, / (H*W), / Wo, / (R*Wo), / QS, / (R*QS)
};

// One launch for a run of consecutive stride-1 inverted-residual blocks on one map, one workgroup per image (f8_irchain.hip): the int8 block
// inputs and the int32 stream between the blocks stay in LDS.  Weights as IRArgs (the fused_ir images), channel counts padded to 32.
struct IRChainBlk {
    const int8_t* w0; const int32_t* b0;   // expand  [E32][cin], offset-corrected bias [E32]
    const int8_t* wd4; const int32_t* bd4; // depthwise: dot4 image [E32/4][36 B], bias (+128*sum(w) for unsigned inputs) [E32]
    const int8_t* w4; const int32_t* b4;   // project [cout][E32], offset-corrected bias [cout]
    int32_t cin, cout, E32;
    Requant r1;                            // requant expand output -> depthwise input format
    Requant r2;                            // requant depthwise output -> project input format
    int32_t relu_a, relu_b, relu0;         // ReLU after expand / depthwise / project
    int32_t res;                           // the block joins its input (int32 stream): (acc << acc_shl) + (stream << res_shl), clamp, ReLU relu1
    int32_t acc_shl, res_shl, relu1;
    Requant rq;                            // requant block output -> the NEXT block's expand input format (all blocks but the last)
    int32_t keep;                          // the next block joins this block's output: it stays in LDS as int32
};
constexpr int kIRChainMaxBlocks = 8;
struct IRChainArgs {
    IRChainBlk blk[kIRChainMaxBlocks]; int32_t nblk;
    int32_t acc_ok;                        // expand / depthwise accumulators of every block bounded (see DwArgs::acc_ok)
    int32_t rq_int;                        // Options::requant_float == 0: integer requantisation only
    const int8_t* x8;                      // first block's input, int8 NHWC [N*H*W][blk[0].cin] in its expand conv's input format
    const int32_t* xr;                     // ... int32 I32T, when blk[0].res
    int32_t N, H, W;
    int32_t* out32; QuantOut q[2];         // forms of the last block's output
    FastDiv dW;                            // / W
    int32_t xp, off_strm, off_patch, off_mid2, off_w;   // LDS layout (filled by launch_irchain)
};

// One launch for a depthwise-separable block: depthwise 3x3 / s, pad 1, ReLU -> 1x1 [ReLU] (f8_dws.hip); int8 outputs only.
struct DwsArgs {
    const int8_t* x;                       // block input, int8 NHWC [N][H][W][Cin] in the depthwise conv's input format
    const int8_t* wd; const int32_t* bd;   // depthwise: [9][Cin] tap-major, bias (+ 128 * sum(w) for unsigned inputs) [Cin]
    const int8_t* w1; const int32_t* b1;   // 1x1: fragment-order image (pack_frag_weights) [Cout][Cin], offset-corrected bias [Cout]
    int32_t N, H, W, P, Q, Cin, Cout, stride;   // H, W: input map; P, Q: output map; channel counts padded to 32
    int32_t R, tiles_per_img, px32;        // output rows per tile (dws_supported); tiles per image and the tile's padded pixel count (launch_dws)
    int32_t in_signed;                     // the depthwise conv reads a signed format (zero padding = 0, else the biased zero)
    Requant r1;                            // requant depthwise output (behind its ReLU) -> the 1x1's input format
    int32_t relu0;                         // ReLU after the 1x1
    QuantOut q[2];
    int32_t acc_ok, rq_int;                // both convs' accumulators bounded (conv_acc_bounded) / Options::requant_float == 0 (see DwArgs)
};

// One launch for a depthwise-separable block whose OUTPUT map is 7 x 7 (f8_dws7.hip): as DwsArgs, the depthwise conv on v_dot4, I images per
// workgroup, and optionally only the average pool of the block output written.
struct Dws7Args {
    const int8_t* x;                       // block input, int8 NHWC [N][H][W][Cin] in the depthwise conv's input format
    const int8_t* wd4; const int32_t* bd4; // depthwise: dot4 image [Cin/4][36 B], bias (+ 128 * sum(w) for unsigned inputs) [Cin]
    const int8_t* w1; const int32_t* b1;   // 1x1: fragment-order image (pack_frag_weights) [Cout][Cin], offset-corrected bias [Cout]
    int32_t N, H, W, Cin, Cout, stride;    // H, W: input map (7 * stride); channel counts padded to 32
    int32_t I, Z, px32;                    // images per workgroup (dws7_supported); slices of the output tiles and the mid tile's padded pixel count (launch_dws7)
    int32_t in_signed;                     // the depthwise conv reads a signed format (zero padding = 0, else the biased zero)
    Requant r1;                            // requant depthwise output (behind its ReLU) -> the 1x1's input format
    int32_t relu0;                         // ReLU after the 1x1
    int32_t pool;                          // the outputs are the forms of the block output SUMMED over its 49 pixels: out32 (I32T, one pixel per image), q (int8 [N][Cout])
    int32_t* out32;
    QuantOut q[2];
    int32_t acc_ok, rq_int;                // both convs' accumulators bounded (conv_acc_bounded) / Options::requant_float == 0 (see DwArgs)
};

// ResNet head in one launch: 7x7/2 conv + ReLU + requant (unsigned 8-bit) + 3x3/2 max-pool (f8_stem.hip).
struct StemPoolArgs {
    int32_t acc_ok;                        // conv accumulators bounded (see DwArgs::acc_ok)
    int32_t rq_int;                        // Options::requant_float == 0: integer requantisation only
    const int8_t* x; uint32_t x_bytes;     // haloed NHWC4 input [N][Hp][Wp][4], halo = conv pad + org pixels
    const int8_t* w; uint32_t w_bytes;     // [64][7][32 B]
    const int32_t* bias;                   // [64], offset-corrected (single class: the halo is biased zero)
    int32_t N, Hp, Wp, org;
    int32_t Pc, Qc, P, Q;                  // conv output size, pooled size
    int32_t relu0;
    int32_t* out32;                        // pooled int32 (I32T, 64 channels) or nullptr
    QuantOut q[2];                         // pooled int8 NHWC (64 channels) in up to two formats
    int32_t wpc;                           // Options::stem_wpc
    int32_t grid_div;                      // Options::stem_grid_div: that kernel runs on 1 / grid_div of the CUs (0 = by output form)
    // h2 != 0: the MobileNet-V2 head instead (3x3 / 2 conv 3 -> 32 ReLU, depthwise 3x3 ReLU, 1x1 32 -> <= 32): w / bias = the head conv
    // ([32][3][32 B], single class), wd / bd = depthwise ([9][32] tap-major, bias + 128 sum(w)), w1 / b1 = the 1x1 ([32][32]); na / nb =
    // right shifts head -> depthwise input / depthwise -> 1x1 input (both unsigned 8-bit behind a ReLU); Pc = P, Qc = Q = its map; q[] only
    int32_t h2; const int8_t* wd; const int32_t* bd; const int8_t* w1; const int32_t* b1; int32_t na, nb;
    // raw network input read by the stem launch itself (no input launch, no haloed NHWC4 copy): NCHW planes, raw_kind 0 = int32 (xi),
    // 1 = fp32 quantised on the fly (xf, scale, qlo, qhi), 2 = uint8 through `lut`; raw_kind < 0: the haloed form `x`
    int32_t raw_kind, rC, rH, rW;
    const int32_t* xi; const float* xf; const uint8_t* xu8;
    float scale; int32_t qlo, qhi;
    uint32_t xor8;                         // 0x80808080 when the stem's input format is unsigned (stored biased)
    uint32_t* err; int32_t chk_lo, chk_hi; // raw_kind 0: values outside [chk_lo, chk_hi] set the sticky error word (err != nullptr)
    int16_t lut[3 * 256];
    // h2 == 2: the MobileNet-V1 form of that head (f8_head_dws.hip, head_dws_kernel): the 1x1 has Cs = 32 or 64 output channels (w1 [Cs][32], b1 [Cs];
    // Cs is also the channel stride of q[]) and carries a ReLU when relu1 is set
    int32_t relu1, Cs;
};

// Dynamic LDS above 64 KB must be opted into per kernel AND per device (a process that drives several GPUs launches the same
// kernel on each of them).  `done`: one static bit mask per call site (bit = device ordinal); a benign race sets the attribute twice.
inline bool dyn_lds_opted_in(unsigned long long* done, int* dev_out) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { *dev_out = -1; return false; }
    *dev_out = dev;
    return ((*done >> dev) & 1ull) != 0;
}

struct ConvTile { int bm, bn, bk; };

// Instances and their names.  A launch family whose launcher chooses between template instances on more than geometry has one
// *_inst function next to its dispatch: f8_net.cpp bind_step calls it once, when the plan is bound, and keeps the value in Step::inst
// (each family defines its bits); the launcher takes that value and only dispatches on it.  *_kernel_name builds the symbol the launcher
// then starts, as rocprofv3 prints it (bench.py joins its live timings with the counter files of profiles/ on that string), next to the
// instantiation; the families whose template argument is the run's raw-input kind are named without their arguments.  nq: the step's
// int8 output forms, q[0 .. nq - 1]; out32 / res: it writes an int32 form / joins an int32 residual operand.

// Tile choice for a conv; returns false if no kernel instance fits (ck % bk).
bool pick_conv_tile(int M, int coutP, int ck, bool has_res, bool bk128, ConvTile* t);
int  conv_grid(const ConvTile& t, int M, int coutP);

int conv_inst(const ConvArgs& a, const ConvTile& t, bool res, bool dual, int deep_nk);   // ring depth (Options::deep_nk), residual, dual GEMM
int conv_kernel_name(char* buf, size_t cap, const ConvArgs& a, const ConvTile& t, int inst);
hipError_t launch_conv(const ConvArgs& a, const ConvTile& t, int inst, hipStream_t s);
hipError_t launch_fused_bottleneck(const FusedArgs& a, hipStream_t s);
int fused_bottleneck_kernel_name(char* buf, size_t cap, const FusedArgs& a);
bool fused_bottleneck_supported(int C, int MID, int H, int W, int imgs_per_launch, int stage_mask, int* R);
bool fused_ds_supported(int C, int MID, int COUT, int H, int W, int* R);
// stage-opening block with a stride-2 3x3 (f8_opener.hip); H, W = input map
bool fused_opener_supported(int C, int MID, int COUT, int H, int W, int* R);
int fused_opener_inst(const FusedArgs& a, bool stg);            // full block: STG (Options::opener_stg); P12 form (p12only): FQ
int fused_opener_kernel_name(char* buf, size_t cap, const FusedArgs& a, int inst);
hipError_t launch_fused_opener(const FusedArgs& a, int inst, hipStream_t s);
// all consecutive bottleneck blocks of a stage in one launch, residual stream in registers (f8_chain.hip).  cin0 != C: the first
// block is the stage-opening block at unchanged resolution (1x1 shortcut conv from cin0 channels).
bool chain_supported(int C, int MID, int H, int W, int cin0);
bool chain_tail_supported(int C, int MID, int H, int W, int cin0);   // ... a stride-2 opening block's join as the first block (H, W = the stage's resolution)
int chain_max_blocks(int C, int MID, int H, int W, int cin0, bool tail);
// rows per tile (4, or 2: the two-workgroups-per-CU instance of tuning builds, -DF8_CH_R2_S0=1) and resident workgroups per CU of the instance that runs the shape
void chain_shape(int C, int MID, int H, int W, int cin0, bool tail, int* R, int* wg_per_cu);
bool chain_stackable(int C, int MID, int H, int W, int cin0, bool tail);   // the instance can tile image pairs as one 2H-row map (ChainArgs::stack = 2)
hipError_t launch_chain(const ChainArgs& a, int fast, int C, int MID, int H, int W, int cin0, hipStream_t s);   // fast: chain_fast (the chain's inst)
int chain_kernel_name(char* buf, size_t cap, int C, int MID, int H, int W, int cin0, bool tail, int fast);   // the symbol launch_chain starts (f8_chain.hip)
// the identity blocks of a 7x7 bottleneck stage over clusters of eight workgroups (f8_cchain.hip): reached through chain_supported / launch_chain
bool cchain_supported(int C, int MID, int H, int W, int cin0, bool tail);   // tail: the join of the stride-2 opening block as the first block (cin0 = its input channels)
size_t cchain_xchg_bytes();                                      // exchange scratch of a launch (per arena copy)
int cchain_clusters(int N, int slots);                           // clusters (ChainArgs::NG) a launch over N images starts on `slots` compute units
int cchain_kernel_name(char* buf, size_t cap, int fast);
int chain_fast(const ChainArgs& a, unsigned shortcut_blocks, bool q8);   // f8_chain.hip: 0 = generic instance, 1 = float-converter requantisation, 2 = integer
hipError_t launch_cchain(const ChainArgs& a, int fast, hipStream_t s);
// consecutive BasicBlocks of a 7x7 x 512 stage over clusters of eight workgroups (f8_bcchain.hip): geometry and clusters as the 7x7 cluster chain (cchain_clusters)
bool bcchain_supported(int C, int H, int W, bool opener);       // opener: the join of the stride-2 opening block first
size_t bcchain_xchg_bytes();
int bcchain_inst(const BCChainArgs& a, bool q8);                 // 2: integer ReLU / unsigned / right-shift instance, 0: any format
int bcchain_kernel_name(char* buf, size_t cap, int inst);
hipError_t launch_bcchain(const BCChainArgs& a, int inst, hipStream_t s);
// consecutive BasicBlock identity blocks of a stage in one launch (f8_bchain.hip)
bool bchain_supported(int C, int H, int W);
bool bchain_ds_supported(int C, int H, int W);
int bchain_tiles_per_img(int C, int H, int W);
hipError_t launch_bchain(const BChainArgs& a, int fast, int C, int H, int W, hipStream_t s);   // fast: bchain_fast
int bchain_fast(const BChainArgs& a, bool ds, bool q8);
int bchain_kernel_name(char* buf, size_t cap, int C, int H, int W, bool ds, int fast);                         // the symbol launch_bchain starts (f8_bchain.hip)
// 1x1 -> 3x3 of a 7x7 bottleneck block in one launch (f8_p12.hip); FusedArgs: x8, w0 / b0, w2 / b2, requant 1, q[] = the int8 outputs
bool fused_p12_supported(int C, int MID, int H, int W);
hipError_t launch_fused_p12(const FusedArgs& a, hipStream_t s);
int fused_p12_kernel_name(char* buf, size_t cap, const FusedArgs& a);
// 1x1 conv with the weights streamed into registers (f8_wreg.hip); ConvArgs::w = the fragment-order image of the weights
bool conv1x1_wreg_supported(int ck, int coutP);
hipError_t launch_conv1x1_wreg(const ConvArgs& a, hipStream_t s);
int conv1x1_wreg_kernel_name(char* buf, size_t cap, const ConvArgs& a);
// classifier: integer linear + int32 -> float32 / int32 [N][classes] into the caller's buffer (f8_fc.hip); ConvArgs::w = fragment order
bool fc_dense_supported(int ck, int coutP);
hipError_t launch_fc_dense(const ConvArgs& a, void* out, int classes, int as_float, const uint32_t* err, uint32_t epoch, hipStream_t s);   // err / epoch: the run's chain error word and tag (logits poisoned when the word carries the tag) or nullptr
int fc_dense_kernel_name(char* buf, size_t cap, const ConvArgs& a);
// 3x3 / stride 2 / pad 1 with the input patch in LDS and the weights streamed into registers (f8_s2conv.hip); ConvArgs::w = fragment order
bool conv3x3s2_wreg_supported(int ck, int HO, int WO, int coutP);
hipError_t launch_conv3x3s2_wreg(const ConvArgs& a, hipStream_t s);
int conv3x3s2_wreg_kernel_name(char* buf, size_t cap, const ConvArgs& a);
// weight-stationary 1x1 conv / dual GEMM / residual join (f8_wstat.hip); ConvArgs::w (and w2) = fragment-order images
bool conv1x1_wstat_supported(int k0, int k1, int coutP, bool has_res);
int conv1x1_wstat_waves(int k0, int k1);
int conv1x1_wstat_inst(const ConvArgs& a, bool res, bool out32, int nq, bool fast);   // fast: Options::wstat_fast
int conv1x1_wstat_kernel_name(char* buf, size_t cap, const ConvArgs& a, int inst);
hipError_t launch_conv1x1_wstat(const ConvArgs& a, int inst, int num_cu, int grid_div, hipStream_t s);   // grid_div: Options::wstat_grid_div
// MobileNet-V2 inverted residual (f8_ir.hip): instance for the padded channel pair + a tile (R rows or G whole images) that fits LDS
bool fused_ir_config(int cinS, int coutS, int H, int W, int stride, int* R, int* G);
int fused_ir_inst(const IRArgs& a, int coutS);
int fused_ir_kernel_name(char* buf, size_t cap, int cinS, int coutS, int inst);
hipError_t launch_fused_ir(const IRArgs& a, int cinS, int coutS, int inst, hipStream_t s);
// inverted residual around a depthwise 5x5 / 7x7, pad K / 2 (f8_irk.hip): padded channel counts; the tile (R rows, or G whole images) that fits LDS
bool irk_supported(int K, int cinS, int coutS);
bool irk_config(int K, int cinS, int coutS, int H, int W, int stride, int* R, int* G);
int irk_inst(const IRKArgs& a);                                    // 2: integer ReLU / unsigned / right-shift instance, 0: any format
int irk_kernel_name(char* buf, size_t cap, int K, int coutS, int inst);
hipError_t launch_fused_irk(const IRKArgs& a, int inst, hipStream_t s);
// a run of stride-1 inverted residuals in one launch (f8_irchain.hip): H x W map, the largest padded block input / output and the widest int32
// stream a later block joins (keep_max; 0: none)
bool irchain_supported(int H, int W, int cin_max, int cout_max, int keep_max);
int irchain_inst(const IRChainArgs& a);                            // FQ (as fused_ir_inst) | register shape << 2
int irchain_kernel_name(char* buf, size_t cap, int inst);
hipError_t launch_irchain(const IRChainArgs& a, int inst, hipStream_t s);
// depthwise-separable block in one launch (f8_dws.hip): padded channel counts, the block INPUT map, the largest N a launch may cover; *R = output rows per tile
bool dws_supported(int cinS, int coutS, int H, int W, int stride, int imgs, int* R);
int dws_inst(const DwsArgs& a, int nq);                            // FQ (0 any format, 1 float converter, 2 integer) | the walker's sub-rows << 2
int dws_kernel_name(char* buf, size_t cap, const DwsArgs& a, int inst);
hipError_t launch_dws(const DwsArgs& a, int inst, hipStream_t s);
// ... whose output map is 7 x 7 (f8_dws7.hip): pool = the launch writes only the average pool of the block output; *I = images per workgroup
bool dws7_supported(int cinS, int coutS, int H, int W, int stride, int imgs, bool pool, int* I);
int dws7_slices(int groups, int nco, int cus);                     // Z: in how many slices the output tiles go over workgroups
int dws7_inst(const Dws7Args& a, int nq);                          // FQ (0 any format, 1 float converter, 2 integer)
int dws7_kernel_name(char* buf, size_t cap, const Dws7Args& a, int inst);
hipError_t launch_dws7(const Dws7Args& a, int inst, int num_cu, hipStream_t s);
// 3x3 / stride 1 / pad 1 with the input patch resident in LDS (f8_conv3x3.hip); config = false: no instance
bool conv3x3_patch_config(int cin, int H, int W, int coutP, int* R, int* IMGS, int* BN);
hipError_t launch_conv3x3_patch(const ConvArgs& a, int cin, hipStream_t s);
int conv3x3_patch_kernel_name(char* buf, size_t cap, int cin, int W, bool res);
bool head2_supported(int H, int W);
int dwconv_mma_inst(const DwArgs& a, bool out32, int nq, int N);   // f8_dwmma.hip: FQ | sub-rows << 2, or -1 (no instance for N images)
hipError_t launch_dwconv_mma(const DwArgs& a, int inst, hipStream_t s);
bool stem_pool_supported(int cin, int cout, int k, int stride, int pad, int pool_k, int pool_s, int pool_p, int P, int Q, int rows, int H, int W);
int stem_pool_inst(const StemPoolArgs& a, bool rows, bool raw);    // 0 tile kernel, 1 row-walking kernel, 2 MobileNet-V2 head, 3 MobileNet-V1 head + block (h2 == 2); raw: the plan reads the raw input
const char* stem_pool_kernel_name(int inst);
hipError_t launch_stem_pool(const StemPoolArgs& a, int inst, hipStream_t s);
// instance 3 (f8_head_dws.hip): dispatched by launch_stem_pool
const char* head_dws_kernel_name();
hipError_t launch_head_dws(const StemPoolArgs& a, hipStream_t s);
// mma / dot4: Options::dw_mma / dw_dot4; max_batch: the largest N a launch may cover (the MMA kernel's 32-bit index bound)
int dwconv_inst(const DwArgs& a, bool out32, int nq, bool mma, bool dot4, int max_batch);
int dwconv_kernel_name(char* buf, size_t cap, const DwArgs& a, int inst);
hipError_t launch_dwconv(const DwArgs& a, int inst, hipStream_t s);
// general depthwise (f8_dwk.hip): every accepted depthwise geometry but the undilated 3x3 / pad 1.  inst 1: dwconvk_dot4_kernel<k, stride> (int8 outputs only,
// Options::dwk_dot4), 2: dwconv3x3_dil_dot4_kernel (the same, 3x3 at dilation > 1, stride 1), 0: dwconvk_kernel<in_signed>
int dwk_inst(const DwArgs& a, bool out32, bool dot4);
int dwk_kernel_name(char* buf, size_t cap, const DwArgs& a, int inst);
hipError_t launch_dwk(const DwArgs& a, int inst, hipStream_t s);
// grouped 3x3 on the slice-diagonal MFMA kernel (f8_gconv.hip): the tile of a P x Q output map (R rows x TW columns, or G whole images)
void gconv_tile(int P, int Q, int stride, int* R, int* TW, int* G);
int gconv_kernel_name(char* buf, size_t cap, const GConvArgs& a);
hipError_t launch_gconv(const GConvArgs& a, hipStream_t s);
int maxpool_inst(const PoolArgs& a);
const char* maxpool_kernel_name(int inst);
hipError_t launch_maxpool(const PoolArgs& a, int inst, hipStream_t s);
const char* avgpool_kernel_name();
hipError_t launch_avgpool(const AvgArgs& a, hipStream_t s);
// last 1x1 conv (+ residual join) + average pool in one launch (f8_pool.hip); ConvArgs::w = fragment order, out32 / q[] = the POOLED forms [N][coutP]
bool conv1x1_pool_supported(int ck, int coutP, int pq);
hipError_t launch_conv1x1_pool(const ConvArgs& a, hipStream_t s);
int conv1x1_pool_kernel_name(char* buf, size_t cap, const ConvArgs& a, bool res);
const char* add_kernel_name();
hipError_t launch_add(const AddArgs& a, hipStream_t s);
int input_inst(int C, int W, bool stem_only);                      // 1: input_stem4_kernel (the input's only form is the stem's NHWC4 copy), 0: input_kernel
const char* input_kernel_name(int inst);
int concat_inst(const ConcatArgs& a, bool i8);                     // f8_concat.hip.  0: concat_i32_kernel, 1: concat_i8_kernel<true> (16-byte vectors), 2: concat_i8_kernel<false>
const char* concat_kernel_name(int inst);
hipError_t launch_concat(const ConcatArgs& a, int inst, hipStream_t s);
int upsample_inst(bool bilinear, bool i8);                         // f8_upsample.hip.  0: upsample_i8_kernel, 1: upsample_i32_kernel<false> (nearest), 2: upsample_i32_kernel<true> (bilinear)
const char* upsample_kernel_name(int inst);
hipError_t launch_upsample(const UpsampleArgs& a, int inst, hipStream_t s);
int deconv_inst(const DeconvArgs& a);                              // f8_deconv.hip.  The cout tiles per wave: 2 (deconv_kernel<2>, coutP >= 64) or 1 (deconv_kernel<1>)
const char* deconv_kernel_name(int inst);
hipError_t launch_deconv(const DeconvArgs& a, int inst, hipStream_t s);
int chanmap_inst(const ChanMapArgs& a, bool i8);                   // f8_chanmap.hip.  0: chanmap_i32_kernel, 1 / 2: slice_i8_kernel<true> / <false>, 3 / 4 / 5: shuffle_i8_kernel<16> / <4> / <2>, 6: shuffle_i8_general_kernel
const char* chanmap_kernel_name(int inst);
hipError_t launch_chanmap(const ChanMapArgs& a, int inst, hipStream_t s);
int pixmap_inst(const PixMapArgs& a, bool i8);                     // f8_pixmap.hip.  0: pixmap_i32_kernel, 1: pixmap_run_i8_kernel (DCR order, runs of a multiple of 16 channels), 2: pixmap_i8_general_kernel, 3 / 4: pixmap_crd2_i8_kernel<false> / <true> (CRD order, r = 2, a multiple of 4 channels; depth_to_space / space_to_depth)
const char* pixmap_kernel_name(int inst);
hipError_t launch_pixmap(const PixMapArgs& a, int inst, hipStream_t s);
int mul_inst(const MulArgs& a, int mode);                          // f8_mul.hip.  mode 0: the stand-alone hard gate, 1: a mul that writes the int32 form, 2: int8 outputs only.  0: hgate_kernel; 1 .. 4: mul_i32_kernel<BCAST, GATE> = <0,0> <0,1> <1,0> <1,1>; 5 .. 10: mul_i8_kernel<BCAST, GATE, V> = <0,0,16> <0,0,4> <1,0,16> <1,0,4> <1,1,16> <1,1,4>
const char* mul_kernel_name(int inst);
int mul_vector_bytes(int inst);                                    // bytes of one operand a lane of the instance owns per step (16 / 4)
hipError_t launch_mul(const MulArgs& a, int inst, hipStream_t s);
constexpr int kTableReplicas = 1;                                  // copies of a byte table in LDS, lane l reads copy l % R (measured, profiles/table_r15.md: 1 is as fast as or faster than 4 and 16 on every shape)
int table_inst(const TableArgs& a, bool i8);                       // f8_table.hip.  0: table_i32_kernel, 1 / 2: table_i8_kernel<16, R> / <4, R>
const char* table_kernel_name(int inst);
hipError_t launch_table(const TableArgs& a, int inst, hipStream_t s);
int table_mul_inst(const TableMulArgs& a, bool i8);                // 0: table_chmul_i32_kernel, 1 / 2: table_chmul_i8_kernel<16> / <4>
const char* table_mul_kernel_name(int inst);
hipError_t launch_table_mul(const TableMulArgs& a, int inst, hipStream_t s);
int sumpool_inst(int k, bool wide);                                // f8_sumpool.hip.  0: sumpool_i32_kernel<0> (kernel size at run time), 2 / 3: sumpool_i32_kernel<2> / <3>, 4: sumpool_wide_kernel
const char* sumpool_kernel_name(int inst);
int sumpool_wide_lg(int k);
hipError_t launch_sumpool(const SumPoolArgs& a, int inst, hipStream_t s);
hipError_t launch_input(const InArgs& a, int inst, hipStream_t s);
const char* output_kernel_name();
hipError_t launch_output(const OutArgs& a, hipStream_t s);
const char* tap_kernel_name(int as_float);                       // f8_tap.hip: the same conversion, one wave per 4 KB block of the I32T source
hipError_t launch_tap(const OutArgs& a, hipStream_t s);
int argmax_inst(bool fused, bool bilinear, int index_bytes);     // f8_argmax.hip.  0 / 1: argmax_i32t_kernel<1> / <4>; 2 / 3: upsample_argmax_kernel<false, 1> / <false, 4>; 4 / 5: upsample_argmax_kernel<true, 1> / <true, 4>
const char* argmax_kernel_name(int inst);
hipError_t launch_argmax(const ArgmaxArgs& a, int inst, hipStream_t s);
hipError_t launch_quantize_input(const float* x, int32_t* y, size_t n, float scale, int lo, int hi, hipStream_t s);
struct TopkKs { int k[8]; };                // the k list travels by value in the kernel arguments
hipError_t launch_topk_correct(const float* logits, const int64_t* target, int N, int C, TopkKs ks, int nk, float* correct, hipStream_t s);
hipError_t launch_requant_i32(const int32_t* src, int32_t* dst, size_t n, int sh, int lo, int hi, hipStream_t s);
hipError_t launch_relu_i32(int32_t* x, size_t n, hipStream_t s);
hipError_t launch_add_align_i32(int32_t* res, const int32_t* x, size_t n, int res_shl, int x_shl, hipStream_t s);

}  // namespace f8
