// f8_net.cpp — graph builder, planner and executor behind include/f8net.h.
//
// The builder records the reference-level integer graph (IntModel.forward,
// /root/reference/models/fix_resnet.py:352-383 and siblings).  f8_net_finalize turns it into a list
// of kernel launches:
//   * every conv's input requantisation (int_op_only_fix_quant, fix_quant_ops.py:90-114) moves into
//     the epilogue of the tensor's PRODUCER, which then emits int8 NHWC in the consumer's format
//     (up to two formats per producer; further ones fall back to a stand-alone requant launch);
//   * ReLU and the residual align-add-clamp (fix_resnet.py:40-54,77) ride in the conv epilogue;
//   * tensors keep an int32 NHWC form only where the reference semantics need 32 bits
//     (residual operands, pooling inputs, network outputs);
//   * a max-pool whose result is only consumed in one int8 format runs on int8 (requant is monotone,
//     so it commutes with max exactly).
// Planning touches no device, so it runs (and is tested) without a GPU.
#include "../../include/f8net.h"
#include "f8_internal.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <variant>
#include <string>
#include <mutex>
#include <vector>

using namespace f8;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    return fail(F8_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline size_t round_up_z(size_t v, size_t m) { return (v + m - 1) / m * m; }

enum FormKind { FORM_I32 = 0, FORM_I8 = 1, FORM_STEM = 2 };
struct Form {
    int kind; int n; int sgn;          // I8: requant shift + signedness of the consumer format
    size_t bytes_per_img = 0;
    size_t slack = 0;                  // I32T: rows padded to a multiple of 32 pixels
    size_t off = 0;                    // arena offset (max_batch sized)
    int first = -1, last = -1;         // step lifetime
    int Hp = 0, Wp = 0, pad = 0;       // STEM
};
struct Tensor {
    int C = 0, H = 0, W = 0, Cs = 0, fl = 0;
    int prod = -1;
    int64_t amax = -2;                 // tensor_amax(), cached (-2: not computed yet)
    std::vector<int> consumers;        // node ids
    std::vector<Form> forms;
    std::string label;
    bool dense_out = false;            // written straight to the caller's output buffer
};
// A fused block: the convs ONE launch (or one block of a chain launch) runs, by role — body.0 / body.2 / body.4 and the shortcut (node ids, -1: the
// block has none).  It is recorded on its HOST, the conv at whose place in node order the launch is emitted and which is one of the roles itself; the
// other convs are its members (Node::absorbed_by = the host; a dual GEMM's other conv: Node::dual_host).  A conv hosts at most one block and is a
// member of at most one (set_block).
//   B_BOTTLENECK    identity bottleneck: 1x1, 3x3, host = body.4 (f8_fused.hip; R = 0: only a chain launch can run it)
//   B_OPENING       stage-opening bottleneck: 1x1, 3x3, body.4 = host.dual, host = shortcut (DS on f8_fused.hip; s2: the stride-2 opener, f8_opener.hip)
//   B_JOIN          its join alone, the FIRST block of a stage chain (ChainArgs::tail): body.4 = host.dual, host = shortcut
//   B_P12           1x1 -> 3x3 in one launch: 1x1, host = the 3x3 (f8_p12.hip; s2: body.0 + body.2 of a stride-2 opening block on f8_opener.hip, whose join opens the chain)
//   B_BASIC         BasicBlock of a chain launch: first 3x3, host = the second 3x3
//   B_BASIC_OPENING stage-opening BasicBlock that opens such a launch: 3x3 / 2, second 3x3, host = the 1x1 / 2 shortcut
//   B_BASIC_JOIN    its join alone (the cluster launch; its 3x3 / 2 runs on its own): second 3x3, host = shortcut
//   B_IR            inverted residual: expand, depthwise, host = project (alone: f8_ir.hip, tile R x G; in a chain launch: f8_irchain.hip)
//   B_IRK           inverted residual around a depthwise 5x5 / 7x7 (option fuse_irk, f8_irk.hip; tile R x G): expand, depthwise, host = project
//   B_HEAD2         MobileNet-V2 head launch (f8_stem.hip, H2): 3x3 / 2 head conv, depthwise, host = the 1x1
//   B_DWS           depthwise-separable block (option fuse_dws, f8_dws.hip; R rows per tile): body.0 = the depthwise 3x3, host = the 1x1;
//                   I7 > 0: the form for a 7 x 7 output map (option fuse_dws7, f8_dws7.hip; I7 images per workgroup), the same block to every pass
enum BlockKind { B_NONE, B_BOTTLENECK, B_OPENING, B_JOIN, B_P12, B_BASIC, B_BASIC_OPENING, B_BASIC_JOIN, B_IR, B_HEAD2, B_DWS, B_IRK };
struct Block { BlockKind kind = B_NONE; int b0 = -1, b2 = -1, b4 = -1, sc = -1; bool s2 = false; int R = 0, G = 0, I7 = 0; };
enum Role { R_NONE, R_B0, R_B2, R_B4, R_SC };
// The chain launches: bottleneck stage (f8_chain.hip; the 7x7 stage over clusters, f8_cchain.hip), BasicBlocks (f8_bchain.hip), BasicBlocks of a 7x7 x 512
// stage over clusters of eight workgroups (option fuse_bchain7, f8_bcchain.hip), inverted residuals (f8_irchain.hip).  Independent of the block kind.
enum ChainKind { C_NONE, C_STAGE, C_BASIC, C_BASIC_CLUSTER, C_IR };
// N_DECONV (f8_net_conv_transpose at stride >= 2) is a kind of its own, not a flag on N_CONV: every matcher asks `kind == N_CONV` and so never sees it — a
// launch of its own (f8_deconv.hip), no block, no chain, no join in its epilogue.  It READS like a conv: its source's int8 form in its consumer format.
// N_SUMPOOL (f8_net_avgpool_window, except the global window, which is N_AVGPOOL) is a kind of its own: no matcher counts it among a block's readers, so
// its source exists in device memory and cuts a chain or fused block where an output tap does.  It reads its source's int32 form.
// N_SLICE / N_SHUFFLE (f8_net_slice, f8_net_channel_shuffle; f8_chanmap.hip) are kinds of their own for the same reason: their source exists in device
// memory and cuts a chain or fused block where an output tap does.  Channel gathers without arithmetic; the mode rule of the nearest upsample.
// N_MUL / N_HGATE (f8_net_mul, f8_net_hard_gate; f8_mul.hip) likewise: a mul READS like a conv — each operand's int8 form in the mul's format for it, written
// by the operand's producer — and a hard gate reads its source's int32 form; no matcher counts either among a block's readers.
// N_TABLE (f8_net_table; f8_table.hip) reads like a conv too — its source's int8 form in the format the table is indexed in — and cuts likewise.
// N_D2S / N_S2D (f8_net_depth_to_space, f8_net_space_to_depth; f8_pixmap.hip) are gathers like N_SLICE / N_SHUFFLE, with their mode rule, and cut likewise.
enum NodeKind { N_INPUT, N_CONV, N_ADD, N_MAXPOOL, N_AVGPOOL, N_LINEAR, N_CONCAT, N_UPSAMPLE, N_DECONV, N_SUMPOOL, N_SLICE, N_SHUFFLE, N_MUL, N_HGATE, N_TABLE, N_D2S, N_S2D };
struct Node {
    int kind; int a = -1, b = -1; int out = -1;
    f8_conv_desc cd{};                 // conv / linear (as 1x1 conv)
    int dil = 1;                       // dilation (f8_net_conv_dilated; 1 for kernel 1).  > 1: a launch of its own on conv_igemm_kernel / f8_dwk.hip — every matcher refuses it
    bool rect = false;                 // f8_net_conv_rect with a geometry that is not square + symmetric: cd.kernel / stride / pad are 0 — no matcher, stem or
    f8_conv_geom rg{};                 // LDS-patch / register-weight variant takes it — and the geometry is rg (geom_of); a launch of its own as a dilated conv
    std::vector<int8_t> w; std::vector<int32_t> bias;   // raw OIHW int8 + bias (N_DECONV: [cin][cout][k][k], nn.ConvTranspose2d's layout)
    int out_pad = 0;                   // N_DECONV: output_padding
    DeconvPhase dph[kMaxDeconvPhases]{};   // N_DECONV: the phase table (pack_deconv_weights; w_off relative to Node::w_off), cd.stride^2 entries
    int acc_ok = -1;                   // conv_acc_bounded(), cached
    int64_t acc_max = -2;              // conv_acc_max(), cached (-2: not computed yet)
    int relu = 0;                      // add
    int pk = 0, pstride = 0, ppad = 0; // maxpool
    int shift = 0;                     // avgpool
    std::vector<int> srcs;             // concat: the operands in channel order (tensor ids; a = srcs[0])
    bool bytes_mode = false;           // concat / upsample / slice / shuffle / depth_to_space / space_to_depth, pass 2: the launch moves bytes, its sources are held in the output's int8 formats; false: sources in int32
    int up_mode = 0, up_sh = 1, up_sw = 1;      // upsample: F8_UP_NEAREST / F8_UP_BILINEAR, the scales
    int sum_k = 0, sum_stride = 0, sum_pad = 0;   // sumpool: the window (its fraclen shift is in the output tensor's fl alone)
    bool sum_wide = false;             // sumpool, pass 2: sumpool_wide_kernel (option sumpool_wide); false: the block walker
    int cm_first = 0, cm_groups = 0;   // slice: the first source channel; shuffle: the groups
    int pm_block = 0, pm_order = 0;    // depth_to_space / space_to_depth: the block r and F8_ORDER_DCR / F8_ORDER_CRD
    int cm_cat = -1;                   // shuffle, pass 2: the concat node in front of it whose operands this launch reads itself (option fuse_shuffle), else -1
    f8_mul_desc md{};                  // mul: the operand formats and the ReLU (operands a, b)
    int mul_gate = -1;                 // mul, pass 2: the hard-gate node that produces b and runs inside this launch (option fuse_hgate), else -1
    int gate_into = -1;                // hard gate, pass 2: the mul node whose launch applies it: no launch and no form of its own
    f8_table_desc td{};                // table: the index format and the entries' fraclen
    std::vector<int32_t> table;        // table: the 256 entries, copied at the call
    int mul_table = -1;                // mul, pass 2: the table node that produces b and is looked up inside this launch (option fuse_table), else -1
    int tab_into = -1;                 // table, pass 2: the mul node whose launch looks it up: no launch and no form of its own
    size_t tab_off = 0;                // table / a mul with mul_table, pass 3: its device tables in the weight image (int32 entries, or 256 bytes per int8 form)
    int argmax_k = -1;                 // upsample, pass 2: the argmax output whose launch interpolates this node's result itself (option fuse_argmax): no launch and no form of its own, else -1
    int cat_into = -1;                 // concat, pass 2: the shuffle node whose launch reads this concat's operands: no launch and no form of its own
    // planning
    int fused_into = -1;               // add: conv node that carries it
    int fused_add = -1;                // conv: add node carried
    bool stem = false, depthwise = false;   // depthwise: groups == cin == cout
    bool grouped = false;              // 1 < groups < cin (option grouped): a launch of its own — gconv3x3_kernel (S_GCONV) or the dense expansion (S_CONV, gconv_kernel_applies)
    int absorbed_by = -1;              // conv that runs inside a fused block hosted by ANOTHER conv (node id of that host; set_block)
    Block blk;                         // the fused block this conv hosts (B_NONE: none)
    int sp_pool = -1, sp_conv = -1;      // stem conv <-> max-pool fused into one launch (f8_stem.hip)
    int pool = -1, pool_host = -1;       // 1x1 conv (hosting its residual join or not) <-> the average pool behind it, one launch (f8_pool.hip)
    int chain_into = -1;               // host of a block that runs inside a chain launch: the host of the chain's LAST block
    std::vector<int> chain;            // host of the last block of a chain: the hosts of all its blocks, in order
    ChainKind chain_kind = C_NONE;     // ... and the launch it is
    int dual = -1;                     // 1x1 conv hosting a join whose other operand is ANOTHER 1x1 conv (node id): one dual-GEMM launch
    int dual_host = -1;                // ... and that other conv: the node that carries it
    int p3_R = 0, p3_imgs = 0, p3_bn = 0;   // 3x3 conv on the LDS-patch kernel (p3_R > 0): rows / images per tile, cout tile
    bool no_classes = false;           // pack a single bias class (the consumer kernel pads with real zeros itself)
    size_t w_off = 0, b_off = 0; int coutP = 0, ck = 0, ktot = 0;
    size_t wf_off = 0;                 // second image of the packed weights in MFMA-fragment order (pack_frag_weights), 0 = none
    size_t rc_off = 0, cc_off = 0; int ncc = 0;      // border-class tables (0 = single class)
    ConvTile tile{};
};
// The per-axis geometry of a conv node: a rectangular node's own, else the square one of its desc.  What packs, counts, names and binds a conv of its own
// reads this; the matchers read cd, where a rectangular node shows kernel 0.
static f8_conv_geom geom_of(const Node& n) {
    if (n.rect) return n.rg;
    const f8_conv_desc& d = n.cd;
    return f8_conv_geom{d.kernel, d.kernel, d.stride, d.stride, d.pad, d.pad, d.pad, d.pad, n.dil};
}
enum StepKind { S_INPUT, S_CONV, S_DW, S_ADD, S_MAXPOOL, S_AVGPOOL, S_REQUANT, S_OUTPUT, S_FUSED, S_STEMPOOL, S_IR, S_P12, S_CHAIN, S_BCHAIN, S_HEAD2, S_IRCHAIN, S_DWS, S_DWS7, S_IRK, S_GCONV, S_CONCAT, S_UPSAMPLE, S_DECONV, S_SUMPOOL, S_CHANMAP, S_MUL, S_HGATE, S_TABLE, S_ARGMAX, S_PIXMAP };
// The kernel of a step whose kind has several, chosen once by the step's emitter (pass 3); bind_step, run_step and f8_net_autotune switch on it.
//   S_CONV:  conv_igemm (f8_kernels.hip), the LDS-patch 3x3 (f8_conv3x3.hip), conv1x1_wreg (f8_wreg.hip), conv1x1_wstat (f8_wstat.hip),
//            conv3x3s2_wreg (f8_s2conv.hip), the 1x1 conv + average pool (f8_pool.hip), the classifier fc_dense (f8_fc.hip)
//   S_FUSED: fused_bottleneck (identity or DS, f8_fused.hip) or the stride-2 opener (f8_opener.hip);  S_P12: fused_p12 (f8_p12.hip) or the opener
enum Variant { V_NONE, V_IGEMM, V_PATCH3X3, V_WREG, V_WSTAT, V_S2WREG, V_POOL, V_FC, V_BOTTLENECK, V_P12, V_OPENER };
struct OutSel { int t = -1; int f32 = -1; int f8[2] = {-1, -1}; };
struct Step {
    int kind; int node;
    Variant variant = V_NONE;
    int src_t = -1, src_f = -1;        // main input tensor / form
    int res_t = -1, res_f = -1;        // residual (conv) or second operand (add)
    int src2_t = -1, src2_f = -1;      // dual GEMM: input of the second conv
    // The gather steps keep what they read HERE, with src_t = res_t = src2_t = -1 (select_sources fills it, gather_sources reads it):
    //   cat_t     the source tensors.  S_CONCAT: its K operands in channel order.  S_UPSAMPLE / S_PIXMAP: the one source.  S_CHANMAP: the one source, or the operands
    //             of the concat the shuffle is fused with (Node::cm_cat).
    //   cat_f[k]  one form index per entry of cat_t.  Bytes mode (Node::bytes_mode): cat_f[k][j] = source j in the format of output form out.f8[k], empty
    //             where out.f8[k] < 0.  Otherwise cat_f[0][j] = source j's int32 form and cat_f[1] is empty.
    // Code that asks what a step reads must look at cat_t as well as the three *_t above: layout_arena (lifetimes) and let_stem_read_input (users of the
    // network input) do.  step_chunk / for_each_launch index tensors[src_t] only for S_FUSED and need not.
    std::vector<int> cat_t, cat_f[2];
    OutSel out;
    int acc_shl = 0, res_shl = 0, relu0 = 0, relu1 = 0;
    bool dense = false;
    int out_k = 0;                     // S_OUTPUT / S_ARGMAX: the network output it writes (0: into the run's output_dev, k >= 1: into buffer k of f8_net_set_output_buffers)
    bool raw_input = false;            // S_INPUT: its work is done by the stem launch (S_STEMPOOL with the same flag) unless the run's input is uint8 NHWC
    std::string name;
    std::string kernel;                // device symbol as rocprofv3 prints it: of the instance bind_step chose (the launch family's *_kernel_name)
    double bytes_per_img = 0, bytes_const = 0, ops_per_img = 0;
    double valu_per_img = 0;           // ESSENTIAL vector lane-operations per image (f8_net_launch_valu): what the reference's semantics need once the MFMAs are done
    // the launcher's arguments as far as the plan decides them (bind_step); run_step copies them and adds what the run decides
    std::variant<std::monostate, ConvArgs, StemPoolArgs, FusedArgs, ChainArgs, BChainArgs, BCChainArgs, IRArgs, IRKArgs, IRChainArgs, DwsArgs, Dws7Args, DwArgs, GConvArgs, AddArgs, PoolArgs, AvgArgs, OutArgs, ConcatArgs, UpsampleArgs, ArgmaxArgs, DeconvArgs, SumPoolArgs, ChanMapArgs, PixMapArgs, MulArgs, TableArgs, TableMulArgs> args;
    int inst = 0;                      // the instance the launcher starts (the family's *_inst, f8_internal.h; bind_step)
    // S_CHAIN / S_BCHAIN: geometry, workgroups per image and resident per CU, the 7x7 cluster form (f8_cchain.hip)
    int C = 0, MID = 0, H = 0, W = 0, cin0 = 0, tiles = 0, wg_per_cu = 1; bool cluster = false;
};

}  // namespace

struct f8_net {
    std::vector<Tensor> tensors;
    std::vector<Node> nodes;
    struct Output { int t; int as_float; int idx = 0; };      // idx: 0 = the tensor's values (f8_net_output); F8_IDX_U8 / F8_IDX_I32 = its channel argmax in elements of that many bytes (f8_net_output_argmax)
    std::vector<Output> outs;          // the network outputs in the order of the f8_net_output calls; [0] is the one f8_net_run's output_dev receives
    void* out_bufs[F8_MAX_OUTPUTS - 1] = {};   // caller buffers of outputs 1 .. (f8_net_set_output_buffers): one-shot, consumed by the next run (begin_run)
    bool out_bufs_set = false;
    bool finalized = false;
    int plan_bug = -1;                 // planning: a conv that two fused blocks claimed (set_block); finalize fails on it
    int max_batch = 0;
    Options opt;                       // per-handle tuning (f8_net_set_option); seeded from the environment at create
    int device = -1;                   // HIP device the arena / weights live on (set by f8_net_upload)
    int num_cu = 0;                    // its compute units (0 before upload: 256 assumed)
    int n_copies = 0;                  // arena copies allocated at upload (= opt.split then)
    hipEvent_t input_ready = nullptr;  // one-shot: the next run's first launch also waits for it (f8_net_set_input_ready)
    std::vector<Step> steps;
    std::vector<uint8_t> wblob;
    size_t arena_bytes = 0;
    size_t arena_stride = 0;           // device arena = kMaxParts copies (one per concurrent sub-batch)
    size_t stem_zero_off = 0, stem_zero_bytes = 0; int stem_zero_val = 0;   // halo = biased zero
    // device
    char* d_arena = nullptr; char* d_w = nullptr; bool uploaded = false;
    uint32_t* d_err = nullptr;         // sticky device error words: [0] an int32 input value outside the head's 8-bit format
    uint32_t* h_err = nullptr; uint32_t* h_err_dev = nullptr;   // host-visible mirror of the chain error words (pinned, mapped): read by f8_net_run without a synchronisation
    uint32_t epoch = 0;                // tag of the run being issued (1 .. 2^24 - 1, f8_net_run): chain error words carry it (ChainArgs::epoch)
    char* d_chain = nullptr; size_t chain_stride = 0;   // per arena copy: sync words + halo exchange rows of the stage-chain launches
    hipEvent_t* events = nullptr; int n_events = 0;
    bool aux_shared = false;           // aux[] belong to the per-device pool (ensure_aux), not to this handle
    hipStream_t aux[4] = {nullptr, nullptr, nullptr, nullptr}; hipEvent_t aux_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t lag_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // pipelined submission (f8_net_set_pipelined): fork dependency = the event recorded at the PREVIOUS run's entry
    int pipelined = 0; hipEvent_t start_ev[4] = {nullptr, nullptr, nullptr, nullptr}; int start_idx = 0; int pipe_count = 0; hipStream_t prev_stream = nullptr;
    int alt_idx = 0;                   // pipelined == 2: internal stream / arena copy of the next run
    // hipGraph of one whole run (both sub-batch streams), replayed while (input, output, N, stream) stay the same
    hipGraphExec_t g_exec = nullptr; const void* g_in = nullptr; void* g_out = nullptr; int g_N = 0; hipStream_t g_stream = nullptr; int g_warm = 0;
};

namespace {

// index of tensor t among the network outputs as a VALUE output (f8_net_output), -1: none.  Every output exists in HBM as int32: no fused launch keeps it on chip.
int output_index(const f8_net* net, int t) {
    for (size_t k = 0; k < net->outs.size(); ++k) if (net->outs[k].t == t && !net->outs[k].idx) return (int)k;
    return -1;
}
// ... as an argmax output (f8_net_output_argmax); a tensor may carry one mark of each kind
int argmax_index(const f8_net* net, int t) {
    for (size_t k = 0; k < net->outs.size(); ++k) if (net->outs[k].t == t && net->outs[k].idx) return (int)k;
    return -1;
}
// either mark: what every matcher asks — the tensor leaves the net, so it exists in device memory and cuts a fused launch
bool is_output(const f8_net* net, int t) { return output_index(net, t) >= 0 || argmax_index(net, t) >= 0; }

int add_form(Tensor& t, int kind, int n, int sgn) {
    for (size_t i = 0; i < t.forms.size(); ++i)
        if (t.forms[i].kind == kind && (kind != FORM_I8 || (t.forms[i].n == n && t.forms[i].sgn == sgn))) return (int)i;
    Form f; f.kind = kind; f.n = n; f.sgn = sgn;
    t.forms.push_back(f);
    return (int)t.forms.size() - 1;
}
int find_form(const Tensor& t, int kind, int n, int sgn) {
    for (size_t i = 0; i < t.forms.size(); ++i)
        if (t.forms[i].kind == kind && (kind != FORM_I8 || (t.forms[i].n == n && t.forms[i].sgn == sgn))) return (int)i;
    return -1;
}

int check_t(const f8_net* net, int t, const char* who) {
    if (!net) return fail(F8_ERR_INVALID, "%s: null net", who);
    if (net->finalized) return fail(F8_ERR_STATE, "%s: net already finalized", who);
    if (t < 0 || t >= (int)net->tensors.size()) return fail(F8_ERR_INVALID, "%s: bad tensor id %d", who, t);
    return 0;
}

int new_tensor(f8_net* net, int C, int H, int W, int fl, int prod) {
    Tensor t; t.C = C; t.H = H; t.W = W; t.Cs = round_up(C, 32); t.fl = fl; t.prod = prod;
    net->tensors.push_back(t);
    return (int)net->tensors.size() - 1;
}

// Is every accumulator of this conv provably below 2^31 - 2^16 in magnitude?  |sum w x + b| <= sum |w| * max |x| + |b| with the 8-bit input
// range (255 unsigned / raw, 127 signed).  Then `v + 2^(n-1)` of the reference's int32 arithmetic (fix_quant_ops.py:100-104) cannot wrap for
// n <= 16 and the three-operation float requantisation (requant_u8x4, f8_device.h) is the same function; real nets are 10^2 - 10^3 below
// the limit, a net that is not keeps the integer form (generic kernel instances).  Cached per node.
constexpr int64_t kAccLimit = (int64_t(1) << 31) - (int64_t(1) << 16) - 1;
// max over the output channels of  sum |w| * max |x| + |b|  (-1: no weights to look at)
static int64_t conv_acc_max(Node& nd) {
    if (nd.acc_max != -2) return nd.acc_max;
    int64_t m = -1;
    if (nd.cd.cout > 0 && !nd.w.empty() && nd.w.size() % (size_t)nd.cd.cout == 0) {
        const size_t per = nd.w.size() / (size_t)nd.cd.cout;
        const int64_t xmax = (nd.cd.quant_input && nd.cd.input_signed) ? 127 : 255;
        const size_t kk = (size_t)nd.cd.kernel * nd.cd.kernel;
        m = 0;
        for (int o = 0; o < nd.cd.cout; ++o) {
            int64_t s = 0;
            // a transposed conv's weights are [cin][cout][k][k]; the sum over ALL taps bounds every phase, which sees a subset of them
            for (size_t k = 0; k < per; ++k) { const int v = nd.kind == N_DECONV ? nd.w[((k / kk) * nd.cd.cout + o) * kk + k % kk] : nd.w[(size_t)o * per + k]; s += v < 0 ? -v : v; }
            const int64_t b = o < (int)nd.bias.size() ? (int64_t)nd.bias[o] : 0;
            m = std::max(m, s * xmax + (b < 0 ? -b : b));
        }
    }
    nd.acc_max = m;
    return m;
}
static bool conv_acc_bounded(Node& nd) {
    if (nd.acc_ok >= 0) return nd.acc_ok != 0;
    const int64_t m = conv_acc_max(nd);
    nd.acc_ok = (m >= 0 && m <= kAccLimit) ? 1 : 0;
    return nd.acc_ok != 0;
}
// A bound on the magnitude of every value an int32 tensor can hold, from the graph alone (round 4): a conv's output by conv_acc_max (a ReLU behind
// it only shrinks it), a max-pool's by its input's, an align-add's (fix_resnet.py:56-76: the operand with the smaller fraclen is shifted left) by the
// shifted sum of its operands' — which makes the int32 residual STREAM of a ResNet stage a bounded quantity: real nets sit at 2^20 .. 2^27.  -1 =
// unknown or beyond 2^40 (the network input, pooled sums).  The chain launches requantise the stream through the float converter only below
// kAccLimit (ChainArgs::stream_ok); beyond it `v + 2^(n-1)` may wrap as the reference's int32 add does, and the integer instances run.
int64_t table_amax(const int32_t table[256], bool sgn);      // (the table op's host side, below)
static int64_t tensor_amax(f8_net* net, int t, int depth = 0) {
    if (t < 0 || t >= (int)net->tensors.size() || depth > 256) return -1;
    Tensor& T = net->tensors[t];
    if (T.amax != -2) return T.amax;
    int64_t m = -1;
    if (T.prod >= 0) {
        Node& nd = net->nodes[T.prod];
        if (nd.kind == N_CONV || nd.kind == N_DECONV) m = conv_acc_max(nd);
        else if (nd.kind == N_MAXPOOL) m = tensor_amax(net, nd.a, depth + 1);
        else if (nd.kind == N_ADD) {
            const int64_t a = tensor_amax(net, nd.a, depth + 1), b = tensor_amax(net, nd.b, depth + 1);
            const int sa = T.fl - net->tensors[nd.a].fl, sb = T.fl - net->tensors[nd.b].fl;      // out fraclen = the larger one (f8_net_add)
            constexpr int64_t cap = int64_t(1) << 40;       // the shifted operands stay below 2^41: no int64 overflow (an operand of 2^40 shifted by 31 would wrap)
            if (a >= 0 && b >= 0 && sa >= 0 && sb >= 0 && sa <= 31 && sb <= 31 && a <= (cap >> sa) && b <= (cap >> sb)) m = (a << sa) + (b << sb);
        } else if (nd.kind == N_CONCAT) {                    // max over the operands of the aligned operand, under the same caps
            constexpr int64_t cap = int64_t(1) << 40;
            m = 0;
            for (int x : nd.srcs) {
                const int64_t a = tensor_amax(net, x, depth + 1);
                const int sa = T.fl - net->tensors[x].fl;
                if (a < 0 || sa < 0 || sa > 31 || a > (cap >> sa)) { m = -1; break; }
                m = std::max(m, a << sa);
            }
        } else if (nd.kind == N_UPSAMPLE) {                  // nearest: the source's; bilinear: the weights of an output sum to 4 s^2, under the same cap
            const int64_t a = tensor_amax(net, nd.a, depth + 1);
            const int sa = T.fl - net->tensors[nd.a].fl;     // 0 / 2k + 2
            constexpr int64_t cap = int64_t(1) << 40;
            if (a >= 0 && sa >= 0 && sa <= 31 && a <= (cap >> sa)) m = a << sa;
        } else if (nd.kind == N_SLICE || nd.kind == N_SHUFFLE || nd.kind == N_D2S || nd.kind == N_S2D) {      // a subset / a permutation of the source's values
            m = tensor_amax(net, nd.a, depth + 1);
        } else if (nd.kind == N_MUL) {                       // the product of the two formats' clamp bounds
            m = (int64_t)(nd.md.a_signed ? 127 : 255) * (nd.md.b_signed ? 127 : 255);
        } else if (nd.kind == N_HGATE) {                     // 0 .. 6 * 2^fl (fl <= 28: f8_net_hard_gate)
            m = int64_t(6) << T.fl;
        } else if (nd.kind == N_TABLE) {                     // the reachable entries
            m = table_amax(nd.table.data(), nd.td.in_signed != 0);
        } else if (nd.kind == N_SUMPOOL) {                   // at most kernel^2 taps of the source's bound, under the same cap
            const int64_t a = tensor_amax(net, nd.a, depth + 1);
            const int64_t kk = (int64_t)nd.sum_k * nd.sum_k;
            constexpr int64_t cap = int64_t(1) << 40;
            if (a >= 0 && a <= cap / kk) m = a * kk;
        }
    }
    if (m > (int64_t(1) << 40)) m = -1;
    T.amax = m;
    return m;
}
// ---- the host side of the table op (f8_net_table)
// int_op_only_fix_quant on one value in the library's integer form — requant1 of f8_device.h, the reference's int32 wrap of `v + 2^(n-1)` included
int requant_host(int32_t v, const Requant& r) {
    const int n = r.n, shr = n > 0 ? n : 0, shl = n > 0 ? 0 : -n;
    const uint32_t hm1 = n > 0 ? (1u << (n - 1)) - 1u : 0u;
    const uint32_t odd = n > 0 ? ((uint32_t)v >> n) & 1u : 0u;
    const uint32_t t = (shl >= 32 ? 0u : (uint32_t)v << shl) + hm1 + odd;
    const int64_t q = (int64_t)(int32_t)t >> shr;       // (arithmetic: int32_t -> int64_t sign-extends, >> of a negative int64 is arithmetic on every compiler this builds with)
    return (int)std::min<int64_t>(std::max<int64_t>(q, r.lo), r.hi);
}
// The byte table of one int8 form of a table's result: bt[u] = the stored byte of requant(table[u], r), u = stored source byte ^ 0x80 (0 .. 255 =
// the unsigned index, or the signed index + 128: the entries' own order for either sign).
void compose_byte_table(const int32_t table[256], const Requant& r, uint8_t bt[256]) {
    for (int u = 0; u < 256; ++u) bt[u] = (uint8_t)((uint32_t)requant_host(table[u], r) ^ (r.bias_xor & 0xffu));
}
// max |entry| over the entries an index can reach: all 256 unsigned, 1 .. 255 signed (index -128 never occurs)
int64_t table_amax(const int32_t table[256], bool sgn) {
    int64_t m = 0;
    for (int u = sgn ? 1 : 0; u < 256; ++u) m = std::max<int64_t>(m, std::llabs((int64_t)table[u]));
    return m;
}

static bool stream_bounded(f8_net* net, int t) { const int64_t m = tensor_amax(net, t); return m >= 0 && m <= kAccLimit; }

// shift / clamp of a consumer's int_op_only_fix_quant; validates what the reference asserts
int consumer_format(const Tensor& src, const f8_conv_desc& d, int* n, const char* who) {
    const int maxfl = d.input_signed ? 7 : 8;
    if (d.input_fl < 0 || d.input_fl > maxfl)
        return fail(F8_ERR_INVALID, "%s: input_fl %d outside [0,%d] (fix_quant_ops.py:91-96)", who, d.input_fl, maxfl);
    *n = d.quant_input ? src.fl - d.input_fl : 0;
    if (*n > 30 || *n < -31) return fail(F8_ERR_INVALID, "%s: requant shift %d out of range", who, *n);
    return 0;
}

int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }

void set_q(QuantOut& q, const Form& f) { static_cast<Requant&>(q) = Requant::of(f.n, f.sgn); }   // the format of an int8 output (its pointer: run_step)

}  // namespace

namespace f8 {
struct OptKey { const char* key; const char* env; int Options::*slot; int lo, hi; bool planning; };
static const OptKey kOptKeys[] = {
    {"split", "F8_SPLIT", &Options::split, 1, 4, true},
    {"fuse_blocks", "F8_FUSE_BLOCKS", &Options::fuse_blocks, 0, 1, true},
    {"fuse_stages", "F8_FUSE_STAGES", &Options::fuse_stages, -1, 7, true},
    {"fuse_dual", "F8_FUSE_DUAL", &Options::fuse_dual, 0, 1, true},
    {"fuse_ds", "F8_FUSE_DS", &Options::fuse_ds, 0, 1, true},
    {"fuse_opener", "F8_FUSE_OPENER", &Options::fuse_opener, 0, 1, true},
    {"fuse_fc", "F8_FUSE_FC", &Options::fuse_fc, 0, 1, true},
    {"fuse_stem", "F8_FUSE_STEM", &Options::fuse_stem, 0, 1, true},
    {"fuse_input", "F8_FUSE_INPUT", &Options::fuse_input, 0, 1, true},
    {"fuse_ir", "F8_FUSE_IR", &Options::fuse_ir, 0, 2, true},
    {"fuse_irchain", "F8_FUSE_IRCHAIN", &Options::fuse_irchain, 0, 1, true},
    {"fuse_irk", "F8_FUSE_IRK", &Options::fuse_irk, 0, 1, true},
    {"fuse_dws", "F8_FUSE_DWS", &Options::fuse_dws, 0, 1, true},
    {"fuse_dws7", "F8_FUSE_DWS7", &Options::fuse_dws7, 0, 1, true},
    {"fuse_head_dws", "F8_FUSE_HEAD_DWS", &Options::fuse_head_dws, 0, 1, true},
    {"fuse_head2", "F8_FUSE_HEAD2", &Options::fuse_head2, 0, 1, true},
    {"fuse_p12", "F8_FUSE_P12", &Options::fuse_p12, 0, 1, true},
    {"fuse_chain", "F8_FUSE_CHAIN", &Options::fuse_chain, 0, 1, true},
    {"fuse_tail", "F8_FUSE_TAIL", &Options::fuse_tail, 0, 1, true},
    {"fuse_chain7", "F8_FUSE_CHAIN7", &Options::fuse_chain7, 0, 1, true},
    {"fuse_pool", "F8_FUSE_POOL", &Options::fuse_pool, 0, 1, true},
    {"fuse_bchain", "F8_FUSE_BCHAIN", &Options::fuse_bchain, 0, 2, true},
    {"fuse_bchain7", "F8_FUSE_BCHAIN7", &Options::fuse_bchain7, 0, 2, true},
    {"chain_timeout_ms", "F8_CHAIN_TIMEOUT_MS", &Options::chain_timeout_ms, 0, 1 << 20, false},
    {"chain_stack", "F8_CHAIN_STACK", &Options::chain_stack, 0, 1, true},
    {"wreg", "F8_WREG", &Options::wreg, 0, 1, true},
    {"s2wreg", "F8_S2WREG", &Options::s2wreg, 0, 1, true},
    {"wstat", "F8_WSTAT", &Options::wstat, 0, 1, true},
    {"wstat_min_tiles", "F8_WSTAT_MIN_TILES", &Options::wstat_min_tiles, 0, 1 << 20, true},
    {"wstat_fast", "F8_WSTAT_FAST", &Options::wstat_fast, 0, 1, true},
    {"wstat_grid_div", "F8_WSTAT_GRID_DIV", &Options::wstat_grid_div, 0, 32, false},
    {"patch3x3", "F8_PATCH3X3", &Options::patch3x3, 0, 1, true},
    {"dual_wide", "F8_DUAL_WIDE", &Options::dual_wide, 0, 1 << 30, true},
    {"deep_nk", "F8_DEEP_NK", &Options::deep_nk, 1, 1 << 20, true},
    {"bk128", "F8_BK128", &Options::bk128, 0, 1, true},
    {"igemm_tile", "F8_IGEMM_TILE", &Options::igemm_tile, 0, 4, true},
    {"dw_dot4", "F8_DW_DOT4", &Options::dw_dot4, 0, 1, true},
    {"dw_mma", "F8_DW_MMA", &Options::dw_mma, 0, 1, true},
    {"dwk_dot4", "F8_DWK_DOT4", &Options::dwk_dot4, 0, 1, true},
    {"stem_wpc", "F8_STEM_WPC", &Options::stem_wpc, 1, 8, false},
    {"stem_rows", "F8_STEM_ROWS", &Options::stem_rows, 0, 1, true},
    {"stem_grid_div", "F8_STEM_GRID_DIV", &Options::stem_grid_div, 0, 32, false},
    {"opener_stg", "F8_OPENER_STG", &Options::opener_stg, 0, 1, true},
    {"chunk56", "F8_CHUNK", &Options::chunk56, -1, 1 << 20, false},
    {"chunk28", "F8_CHUNK28", &Options::chunk28, -1, 1 << 20, false},
    {"chunk14", "F8_CHUNK14", &Options::chunk14, -1, 1 << 20, false},
    {"chunk_budget_mb", "F8_CHUNK_BUDGET_MB", &Options::chunk_budget_mb, 1, 1 << 20, false},
    {"chunk_ds", "F8_CHUNK_DS", &Options::chunk_ds, 0, 1, false},
    {"chunk_opener", "F8_CHUNK_OPENER", &Options::chunk_opener, 0, 1, false},
    {"split_streams", "F8_SPLIT_STREAMS", &Options::split_streams, 0, 1, false},
    {"graph", "F8_GRAPH", &Options::graph, 0, 1, false},
    {"stagger", "F8_STAGGER", &Options::stagger, -1, 1 << 20, false},
    {"stagger_pipelined", "F8_STAGGER_PIPELINED", &Options::stagger_pipelined, 0, 1 << 20, false},
    {"check_device", "F8_CHECK_DEVICE", &Options::check_device, 0, 1, false},
    {"check_input_range", "F8_CHECK_INPUT_RANGE", &Options::check_input_range, 0, 1, false},
    {"requant_float", "F8_REQUANT_FLOAT", &Options::requant_float, 0, 1, true},
    {"pipeline_depth", "F8_PIPELINE_DEPTH", &Options::pipeline_depth, 2, 4, false},
    {"arena_copies", "F8_ARENA_COPIES", &Options::arena_copies, 0, 4, true},
    {"shared_streams", "F8_SHARED_STREAMS", &Options::shared_streams, 0, 1, true},
    {"whole_batch_launches", "F8_WHOLE_BATCH_LAUNCHES", &Options::whole_batch_launches, 0, 1, true},
    {"tap_tiled", "F8_TAP_TILED", &Options::tap_tiled, 0, 1, true},
    {"grouped", "F8_GROUPED", &Options::grouped, 0, 2, true},
    {"concat_i8", "F8_CONCAT_I8", &Options::concat_i8, 0, 1, true},
    {"upsample_i8", "F8_UPSAMPLE_I8", &Options::upsample_i8, 0, 1, true},
    {"sumpool_wide", "F8_SUMPOOL_WIDE", &Options::sumpool_wide, 0, 2, true},
    {"chanmap_i8", "F8_CHANMAP_I8", &Options::chanmap_i8, 0, 1, true},
    {"fuse_shuffle", "F8_FUSE_SHUFFLE", &Options::fuse_shuffle, 0, 1, true},
    {"pixmap_i8", "F8_PIXMAP_I8", &Options::pixmap_i8, 0, 1, true},
    {"fuse_hgate", "F8_FUSE_HGATE", &Options::fuse_hgate, 0, 1, true},
    {"table_i8", "F8_TABLE_I8", &Options::table_i8, 0, 1, true},
    {"fuse_table", "F8_FUSE_TABLE", &Options::fuse_table, 0, 2, true},
    {"fuse_argmax", "F8_FUSE_ARGMAX", &Options::fuse_argmax, 0, 1, true},
};
static const OptKey* find_opt(const char* key) {
    if (!key) return nullptr;
    for (const auto& k : kOptKeys) if (!strcmp(k.key, key)) return &k;
    return nullptr;
}
void options_from_env(Options* o) {
    for (const auto& k : kOptKeys) {
        const int v = env_int(k.env, o->*(k.slot));
        o->*(k.slot) = v < k.lo ? k.lo : (v > k.hi ? k.hi : v);
    }
}
int* option_slot(Options* o, const char* key) { const OptKey* k = find_opt(key); return k ? &(o->*(k->slot)) : nullptr; }
}  // namespace f8

extern "C" {

const char* f8_status_string(int s) {
    switch (s) {
        case F8_OK: return "ok";
        case F8_ERR_INVALID: return "invalid argument";
        case F8_ERR_UNSUPPORTED: return "unsupported";
        case F8_ERR_HIP: return "HIP error";
        case F8_ERR_NOMEM: return "out of memory";
        case F8_ERR_STATE: return "bad state";
        default: return "unknown";
    }
}
const char* f8_last_error(void) { return g_err.c_str(); }
int f8_version(void) { return F8NET_VERSION; }
int f8_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

// ------------------------------------------------------------------------------ op level
int f8_requant_i32(const int32_t* src, int32_t* dst, size_t n, int src_fl, int dst_fl, int is_signed, void* stream) {
    if (dst_fl < 0 || dst_fl > (is_signed ? 7 : 8))
        return fail(F8_ERR_INVALID, "f8_requant_i32: fl %d outside [0,%d]", dst_fl, is_signed ? 7 : 8);
    const int sh = src_fl - dst_fl;
    if (sh > 30 || sh < -31) return fail(F8_ERR_INVALID, "f8_requant_i32: shift %d out of range", sh);
    if (n == 0) return F8_OK;
    if (!src || !dst) return fail(F8_ERR_INVALID, "f8_requant_i32: null pointer");
    hipError_t e = launch_requant_i32(src, dst, n, sh, is_signed ? -127 : 0, is_signed ? 127 : 255, (hipStream_t)stream);
    return e == hipSuccess ? F8_OK : hip_fail(e, "f8_requant_i32");
}
int f8_quantize_input_f32(const float* src, int32_t* dst, size_t n, int normalize, int fl, int is_signed, void* stream) {
    if (normalize && (fl < 0 || fl > (is_signed ? 7 : 8)))
        return fail(F8_ERR_INVALID, "f8_quantize_input_f32: fl %d outside [0,%d] (fix_quant_ops.py:66-71)", fl, is_signed ? 7 : 8);
    if (n == 0) return F8_OK;
    if (!src || !dst) return fail(F8_ERR_INVALID, "f8_quantize_input_f32: null pointer");
    hipError_t e = normalize ? launch_quantize_input(src, dst, n, (float)(1 << fl), is_signed ? -127 : 0, is_signed ? 127 : 255, (hipStream_t)stream)
                             : launch_quantize_input(src, dst, n, 255.f, INT32_MIN, INT32_MAX, (hipStream_t)stream);
    return e == hipSuccess ? F8_OK : hip_fail(e, "f8_quantize_input_f32");
}
int f8_topk_correct_f32(const float* logits, const int64_t* target, int N, int classes, const int* ks, int nk, float* correct, void* stream) {
    if (N < 0 || classes < 1 || nk < 1 || nk > 8 || !ks) return fail(F8_ERR_INVALID, "f8_topk_correct_f32: bad arguments");
    for (int k = 0; k < nk; ++k) if (ks[k] < 1 || ks[k] > classes) return fail(F8_ERR_INVALID, "f8_topk_correct_f32: k=%d outside [1,%d]", ks[k], classes);
    if (N == 0) return F8_OK;
    if (!logits || !target || !correct) return fail(F8_ERR_INVALID, "f8_topk_correct_f32: null pointer");
    // the k list is tiny and call-specific: it travels by value in the kernel arguments (no device scratch, no copy)
    TopkKs kv{};
    for (int k = 0; k < nk; ++k) kv.k[k] = ks[k];
    const hipError_t e = launch_topk_correct(logits, target, N, classes, kv, nk, correct, (hipStream_t)stream);
    return e == hipSuccess ? F8_OK : hip_fail(e, "f8_topk_correct_f32");
}
int f8_relu_i32(int32_t* x, size_t n, void* stream) {
    if (n == 0) return F8_OK;
    if (!x) return fail(F8_ERR_INVALID, "f8_relu_i32: null pointer");
    hipError_t e = launch_relu_i32(x, n, (hipStream_t)stream);
    return e == hipSuccess ? F8_OK : hip_fail(e, "f8_relu_i32");
}
int f8_add_align_i32(int32_t* res, const int32_t* x, size_t n, int res_fl, int x_fl, int* out_fl, void* stream) {
    const int d = res_fl - x_fl;
    if (d > 31 || d < -31) return fail(F8_ERR_INVALID, "f8_add_align_i32: fraclen gap %d too large", d);
    if (out_fl) *out_fl = std::max(res_fl, x_fl);
    if (n == 0) return F8_OK;
    if (!res || !x) return fail(F8_ERR_INVALID, "f8_add_align_i32: null pointer");
    hipError_t e = launch_add_align_i32(res, x, n, d < 0 ? -d : 0, d > 0 ? d : 0, (hipStream_t)stream);
    return e == hipSuccess ? F8_OK : hip_fail(e, "f8_add_align_i32");
}

// ------------------------------------------------------------------------------ builder
f8_net* f8_net_create(void) {
    f8_net* net = new (std::nothrow) f8_net();
    if (net) options_from_env(&net->opt);
    return net;
}

int f8_net_set_option(f8_net* net, const char* key, int value) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_set_option: null net");
    const OptKey* k = find_opt(key);
    if (!k) return fail(F8_ERR_INVALID, "f8_net_set_option: unknown key '%s'", key ? key : "(null)");
    if (value < k->lo || value > k->hi) return fail(F8_ERR_INVALID, "f8_net_set_option: %s = %d outside [%d,%d]", key, value, k->lo, k->hi);
    if (k->planning && net->finalized) return fail(F8_ERR_STATE, "f8_net_set_option: '%s' decides the plan; set it before f8_net_finalize", key);
    net->opt.*(k->slot) = value;
    return F8_OK;
}
int f8_net_get_option(const f8_net* net, const char* key, int* value) {
    if (!net || !value) return fail(F8_ERR_INVALID, "f8_net_get_option: null argument");
    // read-only state key: 1 = the host-visible mirror of the chain error words is active (f8_net_run then refuses further runs after a time-out
    // without a synchronisation); 0 = the page-locked allocation failed at upload / not uploaded yet: only f8_net_check reports a time-out
    if (key && !strcmp(key, "err_mirror")) { *value = (net->uploaded && net->h_err) ? 1 : 0; return F8_OK; }
    const OptKey* k = find_opt(key);
    if (!k) return fail(F8_ERR_INVALID, "f8_net_get_option: unknown key '%s'", key ? key : "(null)");
    *value = net->opt.*(k->slot);
    return F8_OK;
}
int f8_net_check(f8_net* net) {
    if (!net || !net->uploaded) return fail(F8_ERR_STATE, "f8_net_check: not uploaded");
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "f8_net_check: hipDeviceSynchronize");
    if (net->d_err) {
        uint32_t w = 0;
        if ((e = hipMemcpy(&w, net->d_err, 4, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "f8_net_check: hipMemcpy");
        if (w) {
            (void)hipMemset(net->d_err, 0, 4);
            return fail(F8_ERR_INVALID, "f8_net_check: an int32 network input held values outside the head's 8-bit format (the reference would feed them to the "
                                        "head conv as they are; this library narrows the input to 8 bits): outputs of that run are invalid.  Option check_input_range = 0 disables the check");
        }
    }
    if (net->h_err) *(volatile uint32_t*)net->h_err = 0u;      // collected below (the device words stay the authority: one per arena copy)
    uint32_t first_w = 0; int first_p = -1;
    for (int p = 0; net->d_chain && p < net->n_copies; ++p) {
        uint32_t w = 0;
        if ((e = hipMemcpy(&w, net->d_chain + (size_t)p * net->chain_stride + kChainErrWord * 4, 4, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "f8_net_check: hipMemcpy");
        if (w) {
            // ticket, workgroups-out counter, halo flags and the error word of this arena copy: re-armed from the host (the device is idle —
            // the synchronize above — and a launch that did not run to completion would have left them dirty).  EVERY copy is collected by this call.
            (void)hipMemset(net->d_chain + (size_t)p * net->chain_stride, 0, 4096);
            if (first_p < 0) { first_w = w; first_p = p; }
        }
    }
    if (first_p >= 0)
        return fail(F8_ERR_HIP, "f8_net_check: a stage-chain launch gave up waiting for a neighbouring tile (code 0x%x of run tag %u, arena copy %d): the outputs of that run are invalid", first_w & 0xffu, first_w >> 8, first_p);
    return F8_OK;
}
int f8_net_set_input_ready(f8_net* net, void* event) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_set_input_ready: null net");
    net->input_ready = (hipEvent_t)event;
    return F8_OK;
}

void f8_net_destroy(f8_net* net) {
    if (!net) return;
    if (net->d_arena) (void)hipFree(net->d_arena);
    if (net->d_w) (void)hipFree(net->d_w);
    if (net->d_chain) (void)hipFree(net->d_chain);
    if (net->d_err) (void)hipFree(net->d_err);
    if (net->h_err) (void)hipHostFree(net->h_err);
    if (net->events) {
        for (int i = 0; i < net->n_events; ++i) (void)hipEventDestroy(net->events[i]);
        delete[] net->events;
    }
    for (int k = 0; k < 4; ++k) if (net->aux[k] && !net->aux_shared) (void)hipStreamDestroy(net->aux[k]);
    for (int k = 0; k < 5; ++k) if (net->aux_ev[k]) (void)hipEventDestroy(net->aux_ev[k]);
    for (int k = 0; k < 4; ++k) if (net->lag_ev[k]) (void)hipEventDestroy(net->lag_ev[k]);
    if (net->g_exec) (void)hipGraphExecDestroy(net->g_exec);
    for (int k = 0; k < 4; ++k) if (net->start_ev[k]) (void)hipEventDestroy(net->start_ev[k]);
    delete net;
}

int f8_net_input(f8_net* net, int C, int H, int W, int fraclen) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_input: null net");
    if (net->finalized) return fail(F8_ERR_STATE, "f8_net_input: finalized");
    if (C <= 0 || H <= 0 || W <= 0) return fail(F8_ERR_INVALID, "f8_net_input: bad shape");
    for (auto& n : net->nodes) if (n.kind == N_INPUT) return fail(F8_ERR_UNSUPPORTED, "f8_net_input: one input per net");
    Node nd; nd.kind = N_INPUT;
    net->nodes.push_back(nd);
    const int t = new_tensor(net, C, H, W, fraclen, (int)net->nodes.size() - 1);
    net->nodes.back().out = t;
    return t;
}

static int push_conv_node(f8_net* net, int src, const f8_conv_desc& d, int dil, const f8_conv_geom* rg, int P, int Q, const int32_t* w, const int32_t* b,
                          int kind, const char* who);
static int add_conv_node(f8_net* net, int src, const f8_conv_desc& d, int dil, const int32_t* w, const int32_t* b,
                         int kind, const char* who) {
    int rc = check_t(net, src, who);
    if (rc) return rc;
    const Tensor& s = net->tensors[src];
    if (d.cin != s.C) return fail(F8_ERR_INVALID, "%s: cin %d != source channels %d", who, d.cin, s.C);
    if (d.kernel < 1 || d.stride < 1 || d.pad < 0 || d.cout < 1) return fail(F8_ERR_INVALID, "%s: bad geometry", who);
    if (dil < 1) return fail(F8_ERR_INVALID, "%s: dilation %d < 1 (kernel %d, stride %d, pad %d)", who, dil, d.kernel, d.stride, d.pad);
    if (dil > 64) return fail(F8_ERR_UNSUPPORTED, "%s: dilation %d > 64 is not built (kernel %d, stride %d, pad %d)", who, dil, d.kernel, d.stride, d.pad);
    if (d.kernel == 1) dil = 1;                   // a 1x1 has no second tap: the same conv
    // grouped convs (1 < groups < cin) are opt-in at the builder (option grouped): planned on f8_gconv.hip or as the dense expansion (emit_conv_family)
    const bool grouped = d.groups > 1 && d.groups < d.cin && net->opt.grouped >= 1;
    if (grouped) {
        if (d.cin % d.groups || d.cout % d.groups) return fail(F8_ERR_INVALID, "%s: groups %d must divide cin %d and cout %d", who, d.groups, d.cin, d.cout);
    } else if (!(d.groups == 1 || (d.groups == d.cin && d.cout == d.cin)))
        return fail(F8_ERR_UNSUPPORTED, "%s: groups must be 1 or cin (depthwise)", who);
    if (d.groups != 1 && !grouped && dil == 1 && !((d.kernel == 3 || d.kernel == 5 || d.kernel == 7) && d.stride <= 2 && d.pad <= d.kernel / 2))
        return fail(F8_ERR_UNSUPPORTED, "%s: depthwise is built for kernel 3, 5 or 7, stride 1 or 2, pad 0 .. kernel / 2 (got kernel %d, stride %d, pad %d)",
                    who, d.kernel, d.stride, d.pad);
    if (d.groups != 1 && !grouped && dil > 1 && !(d.kernel == 3 && d.stride <= 2 && d.pad <= dil))
        return fail(F8_ERR_UNSUPPORTED, "%s: dilated depthwise is built for kernel 3, stride 1 or 2, pad 0 .. dilation (got kernel %d, stride %d, pad %d, dilation %d)",
                    who, d.kernel, d.stride, d.pad, dil);
    if (d.weight_fl < 0 || d.weight_fl > 31) return fail(F8_ERR_INVALID, "%s: bad weight_fl", who);
    int n;
    rc = consumer_format(s, d, &n, who);
    if (rc) return rc;
    const int ext = dil * (d.kernel - 1) + 1;     // the kernel's extent on the input
    if (s.H + 2 * d.pad < ext || s.W + 2 * d.pad < ext) {
        if (dil == 1) return fail(F8_ERR_INVALID, "%s: kernel larger than padded input", who);
        return fail(F8_ERR_INVALID, "%s: empty output: kernel %d at dilation %d spans %d pixels, the padded input is %d x %d (pad %d)", who, d.kernel, dil, ext,
                    s.H + 2 * d.pad, s.W + 2 * d.pad, d.pad);
    }
    const int P = (s.H + 2 * d.pad - ext) / d.stride + 1, Q = (s.W + 2 * d.pad - ext) / d.stride + 1;
    return push_conv_node(net, src, d, dil, nullptr, P, Q, w, b, kind, who);
}

// records a validated conv: the node (rg: the geometry of a rectangular one, else null), its copied weights and its [cout, P, Q] result
static int push_conv_node(f8_net* net, int src, const f8_conv_desc& d, int dil, const f8_conv_geom* rg, int P, int Q, const int32_t* w, const int32_t* b,
                          int kind, const char* who) {
    if (!w) return fail(F8_ERR_INVALID, "%s: null weight", who);
    Node nd; nd.kind = kind; nd.a = src; nd.cd = d; nd.dil = dil;
    if (rg) { nd.rect = true; nd.rg = *rg; }
    const size_t wn = (size_t)d.cout * (d.cin / d.groups) * (rg ? rg->kh * rg->kw : d.kernel * d.kernel);
    nd.w.resize(wn);
    for (size_t i = 0; i < wn; ++i) {
        if (w[i] < -128 || w[i] > 127) return fail(F8_ERR_INVALID, "%s: weight %d does not fit int8", who, w[i]);
        nd.w[i] = (int8_t)w[i];
    }
    nd.bias.assign(d.cout, 0);
    if (b) for (int i = 0; i < d.cout; ++i) nd.bias[i] = b[i];
    net->nodes.push_back(std::move(nd));
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, d.cout, P, Q, d.weight_fl + d.input_fl, id);
    net->nodes[id].out = t;
    net->tensors[src].consumers.push_back(id);
    return t;
}

int f8_net_conv(f8_net* net, int src, const f8_conv_desc* desc, const int32_t* w, const int32_t* b) {
    if (!desc) return fail(F8_ERR_INVALID, "f8_net_conv: null desc");
    return add_conv_node(net, src, *desc, 1, w, b, N_CONV, "f8_net_conv");
}

int f8_net_conv_dilated(f8_net* net, int src, const f8_conv_desc* desc, int dilation, const int32_t* w, const int32_t* b) {
    if (!desc) return fail(F8_ERR_INVALID, "f8_net_conv_dilated: null desc");
    return add_conv_node(net, src, *desc, dilation, w, b, N_CONV, "f8_net_conv_dilated");
}

int f8_net_conv_rect(f8_net* net, int src, const f8_conv_desc* desc, const f8_conv_geom* geom, const int32_t* w, const int32_t* b) {
    const char* who = "f8_net_conv_rect";
    if (!desc) return fail(F8_ERR_INVALID, "%s: null desc", who);
    if (!geom) return fail(F8_ERR_INVALID, "%s: null geom", who);
    if (const int rc = check_t(net, src, who)) return rc;
    f8_conv_desc d = *desc;
    f8_conv_geom g = *geom;
    if (d.kernel || d.stride || d.pad)
        return fail(F8_ERR_INVALID, "%s: desc kernel %d, stride %d, pad %d must be 0: the geometry comes from geom", who, d.kernel, d.stride, d.pad);
    char gs[192];
    snprintf(gs, sizeof gs, "kernel %d x %d, stride (%d, %d), pads (top %d, left %d, bottom %d, right %d), dilation %d", g.kh, g.kw, g.stride_h, g.stride_w,
             g.pad_top, g.pad_left, g.pad_bottom, g.pad_right, g.dilation);
    if (g.kh < 1 || g.kw < 1 || g.kh > 31 || g.kw > 31) return fail(F8_ERR_INVALID, "%s: kernel sides must be 1 .. 31 (%s)", who, gs);
    if (g.stride_h < 1 || g.stride_w < 1) return fail(F8_ERR_INVALID, "%s: strides must be >= 1 (%s)", who, gs);
    if (g.pad_top < 0 || g.pad_left < 0 || g.pad_bottom < 0 || g.pad_right < 0) return fail(F8_ERR_INVALID, "%s: pads must be >= 0 (%s)", who, gs);
    if (g.dilation < 1) return fail(F8_ERR_INVALID, "%s: dilation %d < 1 (%s)", who, g.dilation, gs);
    // square and symmetric: the node f8_net_conv_dilated records, with its rules and messages
    if (g.kh == g.kw && g.stride_h == g.stride_w && g.pad_top == g.pad_left && g.pad_top == g.pad_bottom && g.pad_top == g.pad_right) {
        d.kernel = g.kh; d.stride = g.stride_h; d.pad = g.pad_top;
        return add_conv_node(net, src, d, g.dilation, w, b, N_CONV, who);
    }
    if (g.dilation > 64) return fail(F8_ERR_UNSUPPORTED, "%s: dilation %d > 64 is not built (%s)", who, g.dilation, gs);
    if (g.kh == 1 && g.kw == 1) g.dilation = 1;    // no second tap: the same conv
    const Tensor& s = net->tensors[src];
    if (d.cin != s.C) return fail(F8_ERR_INVALID, "%s: cin %d != source channels %d", who, d.cin, s.C);
    if (d.cout < 1) return fail(F8_ERR_INVALID, "%s: cout %d < 1", who, d.cout);
    const int eh = g.dilation * (g.kh - 1) + 1, ew = g.dilation * (g.kw - 1) + 1;      // the kernel's extent on the input, per axis
    if (g.pad_top >= eh || g.pad_bottom >= eh || g.pad_left >= ew || g.pad_right >= ew)
        return fail(F8_ERR_INVALID, "%s: a pad exceeds its axis' extent - 1 (%d rows, %d columns; %s)", who, eh - 1, ew - 1, gs);
    if (d.groups > 1 && d.groups < d.cin) return fail(F8_ERR_UNSUPPORTED, "%s: grouped rectangular convs are not built (groups %d of cin %d; %s)", who, d.groups, d.cin, gs);
    if (!(d.groups == 1 || (d.groups == d.cin && d.cout == d.cin))) return fail(F8_ERR_UNSUPPORTED, "%s: groups must be 1 or cin (depthwise)", who);
    if (d.groups != 1) {
        const int k = std::max(g.kh, g.kw);
        const bool strip = std::min(g.kh, g.kw) == 1 && k >= 3 && g.dilation == 1 && g.stride_h == g.stride_w && g.stride_h <= 2;
        if (!strip)
            return fail(F8_ERR_UNSUPPORTED, "%s: rectangular depthwise is built for strips only: 1 x k or k x 1 with 3 <= k <= 31, dilation 1, one stride of 1 or 2 (got %s)", who, gs);
    }
    if (d.weight_fl < 0 || d.weight_fl > 31) return fail(F8_ERR_INVALID, "%s: bad weight_fl", who);
    int n;
    if (const int rc = consumer_format(s, d, &n, who)) return rc;
    const int Hp = s.H + g.pad_top + g.pad_bottom, Wp = s.W + g.pad_left + g.pad_right;
    if (Hp < eh || Wp < ew)
        return fail(F8_ERR_INVALID, "%s: empty output: the kernel spans %d x %d pixels, the padded input is %d x %d (%s)", who, eh, ew, Hp, Wp, gs);
    return push_conv_node(net, src, d, g.dilation, &g, (Hp - eh) / g.stride_h + 1, (Wp - ew) / g.stride_w + 1, w, b, N_CONV, who);
}

int f8_net_conv_transpose(f8_net* net, int src, const f8_conv_desc* desc, int output_padding, const int32_t* w, const int32_t* b) {
    const char* who = "f8_net_conv_transpose";
    if (!desc) return fail(F8_ERR_INVALID, "%s: null desc", who);
    const f8_conv_desc& d = *desc;
    if (const int rc = check_t(net, src, who)) return rc;
    const Tensor s = net->tensors[src];
    if (d.cin != s.C) return fail(F8_ERR_INVALID, "%s: cin %d != source channels %d", who, d.cin, s.C);
    if (d.kernel < 1 || d.stride < 1 || d.pad < 0 || d.cout < 1)
        return fail(F8_ERR_INVALID, "%s: bad geometry (kernel %d, stride %d, pad %d, cout %d)", who, d.kernel, d.stride, d.pad, d.cout);
    if (d.groups != 1) return fail(F8_ERR_UNSUPPORTED, "%s: groups %d: only groups == 1 is built", who, d.groups);
    if (d.kernel > 8) return fail(F8_ERR_UNSUPPORTED, "%s: kernel %d > 8 is not built", who, d.kernel);
    if (d.stride > 4) return fail(F8_ERR_UNSUPPORTED, "%s: stride %d > 4 is not built (kernel %d)", who, d.stride, d.kernel);
    if (d.pad > d.kernel - 1) return fail(F8_ERR_UNSUPPORTED, "%s: pad %d > kernel - 1 = %d is not built", who, d.pad, d.kernel - 1);
    if (output_padding < 0 || output_padding >= d.stride)
        return fail(F8_ERR_INVALID, "%s: output_padding %d outside [0, stride %d)", who, output_padding, d.stride);
    if (d.weight_fl < 0 || d.weight_fl > 31) return fail(F8_ERR_INVALID, "%s: bad weight_fl %d", who, d.weight_fl);
    int n;
    if (const int rc = consumer_format(s, d, &n, who)) return rc;
    const int64_t P = (int64_t)(s.H - 1) * d.stride - 2 * d.pad + d.kernel + output_padding, Q = (int64_t)(s.W - 1) * d.stride - 2 * d.pad + d.kernel + output_padding;
    if (P < 1 || Q < 1)
        return fail(F8_ERR_INVALID, "%s: empty output %lld x %lld from a %d x %d map (kernel %d, stride %d, pad %d, output_padding %d)", who, (long long)P, (long long)Q,
                    s.H, s.W, d.kernel, d.stride, d.pad, output_padding);
    if (P > INT32_MAX / 4 || Q > INT32_MAX / 4 || P * Q > INT32_MAX / 4 || P * Q * round_up(d.cout, 32) > INT32_MAX / 4)
        return fail(F8_ERR_UNSUPPORTED, "%s: the %lld x %lld x %d result exceeds 2 GiB per tensor", who, (long long)P, (long long)Q, d.cout);
    if (!w) return fail(F8_ERR_INVALID, "%s: null weight", who);
    const int k = d.kernel;
    const size_t wn = (size_t)d.cin * d.cout * k * k;
    for (size_t i = 0; i < wn; ++i)
        if (w[i] < -128 || w[i] > 127) return fail(F8_ERR_INVALID, "%s: weight %d does not fit int8", who, w[i]);
    if (d.stride == 1) {
        // not a new op: the plain conv with pad' = k - 1 - pad over the weights flipped in both axes and swapped to [cout][cin][k][k]
        std::vector<int32_t> wc(wn);
        for (int ci = 0; ci < d.cin; ++ci)
            for (int co = 0; co < d.cout; ++co)
                for (int r = 0; r < k; ++r)
                    for (int c = 0; c < k; ++c)
                        wc[(((size_t)co * d.cin + ci) * k + (k - 1 - r)) * k + (k - 1 - c)] = w[(((size_t)ci * d.cout + co) * k + r) * k + c];
        f8_conv_desc c = d;
        c.pad = k - 1 - d.pad;
        return add_conv_node(net, src, c, 1, wc.data(), b, N_CONV, who);
    }
    Node nd; nd.kind = N_DECONV; nd.a = src; nd.cd = d; nd.out_pad = output_padding;
    nd.w.resize(wn);
    for (size_t i = 0; i < wn; ++i) nd.w[i] = (int8_t)w[i];
    nd.bias.assign(d.cout, 0);
    if (b) for (int i = 0; i < d.cout; ++i) nd.bias[i] = b[i];
    net->nodes.push_back(std::move(nd));
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, d.cout, (int)P, (int)Q, d.weight_fl + d.input_fl, id);
    net->nodes[id].out = t;
    net->tensors[src].consumers.push_back(id);
    return t;
}

int f8_net_linear(f8_net* net, int src, const f8_linear_desc* d, const int32_t* w, const int32_t* b) {
    if (!d) return fail(F8_ERR_INVALID, "f8_net_linear: null desc");
    int rc = check_t(net, src, "f8_net_linear");
    if (rc) return rc;
    const Tensor& s = net->tensors[src];
    if (s.H != 1 || s.W != 1) return fail(F8_ERR_INVALID, "f8_net_linear: source must be [C,1,1]");
    f8_conv_desc c{};
    c.cin = d->in_features; c.cout = d->out_features; c.kernel = 1; c.stride = 1; c.pad = 0; c.groups = 1;
    c.weight_fl = d->weight_fl; c.input_fl = d->input_fl; c.input_signed = d->input_signed;
    c.quant_input = d->quant_input; c.relu = 0;
    return add_conv_node(net, src, c, 1, w, b, N_LINEAR, "f8_net_linear");
}

int f8_net_add(f8_net* net, int a, int b, int relu) {
    int rc = check_t(net, a, "f8_net_add");
    if (rc) return rc;
    rc = check_t(net, b, "f8_net_add");
    if (rc) return rc;
    const Tensor &ta = net->tensors[a], &tb = net->tensors[b];
    if (ta.C != tb.C || ta.H != tb.H || ta.W != tb.W) return fail(F8_ERR_INVALID, "f8_net_add: shape mismatch");
    if (a == b) return fail(F8_ERR_UNSUPPORTED, "f8_net_add: operands must differ");
    if (std::abs(ta.fl - tb.fl) > 31) return fail(F8_ERR_INVALID, "f8_net_add: fraclen gap too large");
    Node nd; nd.kind = N_ADD; nd.a = a; nd.b = b; nd.relu = relu;
    net->nodes.push_back(nd);
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, ta.C, ta.H, ta.W, std::max(ta.fl, tb.fl), id);
    net->nodes[id].out = t;
    net->tensors[a].consumers.push_back(id);
    net->tensors[b].consumers.push_back(id);
    return t;
}

static_assert(F8_MAX_CONCAT == kMaxConcat, "ConcatArgs holds F8_MAX_CONCAT sources");
int f8_net_concat(f8_net* net, const int* srcs, int n) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_concat: null net");
    if (net->finalized) return fail(F8_ERR_STATE, "f8_net_concat: net already finalized");
    if (!srcs || n < 2) return fail(F8_ERR_INVALID, "f8_net_concat: at least two operands (got %d)", srcs ? n : 0);
    if (n > F8_MAX_CONCAT) return fail(F8_ERR_UNSUPPORTED, "f8_net_concat: at most %d operands (got %d)", F8_MAX_CONCAT, n);
    int C = 0, fl = INT32_MIN, fl_min = INT32_MAX;
    for (int i = 0; i < n; ++i) {
        if (const int rc = check_t(net, srcs[i], "f8_net_concat")) return rc;
        const Tensor &t = net->tensors[srcs[i]], &t0 = net->tensors[srcs[0]];
        if (t.H != t0.H || t.W != t0.W) return fail(F8_ERR_INVALID, "f8_net_concat: operand %d is %d x %d, operand 0 is %d x %d", i, t.H, t.W, t0.H, t0.W);
        C += t.C; fl = std::max(fl, t.fl); fl_min = std::min(fl_min, t.fl);
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (srcs[i] == srcs[j]) return fail(F8_ERR_UNSUPPORTED, "f8_net_concat: operands must differ (tensor %d twice)", srcs[i]);
    if (fl - fl_min > 31) return fail(F8_ERR_INVALID, "f8_net_concat: fraclen gap too large");
    Node nd; nd.kind = N_CONCAT; nd.a = srcs[0]; nd.srcs.assign(srcs, srcs + n);
    net->nodes.push_back(nd);
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, C, net->tensors[srcs[0]].H, net->tensors[srcs[0]].W, fl, id);
    net->nodes[id].out = t;
    for (int i = 0; i < n; ++i) net->tensors[srcs[i]].consumers.push_back(id);
    return t;
}

int f8_net_upsample(f8_net* net, int src, int mode, int scale_h, int scale_w) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_upsample: null net");
    if (net->finalized) return fail(F8_ERR_STATE, "f8_net_upsample: net already finalized");
    if (const int rc = check_t(net, src, "f8_net_upsample")) return rc;
    if (mode != F8_UP_NEAREST && mode != F8_UP_BILINEAR) return fail(F8_ERR_INVALID, "f8_net_upsample: unknown mode %d", mode);
    if (scale_h < 1 || scale_w < 1 || (scale_h == 1 && scale_w == 1))
        return fail(F8_ERR_INVALID, "f8_net_upsample: scales must be >= 1 and not both 1 (got %d, %d)", scale_h, scale_w);
    const Tensor s = net->tensors[src];
    int fl = s.fl;
    if (mode == F8_UP_NEAREST) {
        if (scale_h > 256 || scale_w > 256) return fail(F8_ERR_UNSUPPORTED, "f8_net_upsample: nearest scales above 256 are not built (got %d, %d)", scale_h, scale_w);
    } else {
        if (scale_h != scale_w || (scale_h != 2 && scale_h != 4 && scale_h != 8 && scale_h != 16))
            return fail(F8_ERR_UNSUPPORTED, "f8_net_upsample: bilinear is built for equal scales of 2, 4, 8 or 16 (got %d, %d)", scale_h, scale_w);
        int k = 0;
        while ((1 << k) < scale_h) ++k;
        fl = s.fl + 2 * k + 2;                                 // the weights of an output sum to 4 s^2 = 2^(2k + 2)
        if (fl > 32) return fail(F8_ERR_INVALID, "f8_net_upsample: output fraclen %d > 32", fl);
    }
    if ((int64_t)s.H * scale_h > INT32_MAX / 4 || (int64_t)s.W * scale_w > INT32_MAX / 4 || (int64_t)s.H * scale_h * s.W * scale_w > INT32_MAX / 4)
        return fail(F8_ERR_UNSUPPORTED, "f8_net_upsample: the %d x %d map times (%d, %d) exceeds 2 GiB per tensor", s.H, s.W, scale_h, scale_w);
    Node nd; nd.kind = N_UPSAMPLE; nd.a = src; nd.up_mode = mode; nd.up_sh = scale_h; nd.up_sw = scale_w;
    net->nodes.push_back(nd);
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, s.C, s.H * scale_h, s.W * scale_w, fl, id);
    net->nodes[id].out = t;
    net->tensors[src].consumers.push_back(id);
    return t;
}

int f8_net_slice(f8_net* net, int src, int first, int channels) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_slice: null net");
    if (net->finalized) return fail(F8_ERR_STATE, "f8_net_slice: net already finalized");
    if (const int rc = check_t(net, src, "f8_net_slice")) return rc;
    const Tensor s = net->tensors[src];
    if (first < 0 || channels < 1 || first > s.C || channels > s.C - first)
        return fail(F8_ERR_INVALID, "f8_net_slice: channels [%d, %d + %d) outside the source's %d", first, first, channels, s.C);
    if (channels == s.C) return fail(F8_ERR_INVALID, "f8_net_slice: the whole tensor (%d channels) is the identity: use the source", s.C);
    Node nd; nd.kind = N_SLICE; nd.a = src; nd.cm_first = first;
    net->nodes.push_back(nd);
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, channels, s.H, s.W, s.fl, id);
    net->nodes[id].out = t;
    net->tensors[src].consumers.push_back(id);
    return t;
}

int f8_net_channel_shuffle(f8_net* net, int src, int groups) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_channel_shuffle: null net");
    if (net->finalized) return fail(F8_ERR_STATE, "f8_net_channel_shuffle: net already finalized");
    if (const int rc = check_t(net, src, "f8_net_channel_shuffle")) return rc;
    const Tensor s = net->tensors[src];
    if (groups < 2 || s.C % groups) return fail(F8_ERR_INVALID, "f8_net_channel_shuffle: groups %d must be >= 2 and divide the %d channels", groups, s.C);
    if (groups == s.C) return fail(F8_ERR_INVALID, "f8_net_channel_shuffle: groups == channels (%d) is the identity: use the source", s.C);
    if (groups > F8_MAX_CONCAT) return fail(F8_ERR_UNSUPPORTED, "f8_net_channel_shuffle: at most %d groups (got %d)", F8_MAX_CONCAT, groups);
    Node nd; nd.kind = N_SHUFFLE; nd.a = src; nd.cm_groups = groups;
    net->nodes.push_back(nd);
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, s.C, s.H, s.W, s.fl, id);
    net->nodes[id].out = t;
    net->tensors[src].consumers.push_back(id);
    return t;
}

// depth_to_space (s2d == 0) / space_to_depth (s2d == 1): the checks and the node
static int add_pixmap(f8_net* net, int src, int block, int order, bool s2d) {
    const char* fn = s2d ? "f8_net_space_to_depth" : "f8_net_depth_to_space";
    if (!net) return fail(F8_ERR_INVALID, "%s: null net", fn);
    if (net->finalized) return fail(F8_ERR_STATE, "%s: net already finalized", fn);
    if (const int rc = check_t(net, src, fn)) return rc;
    if (block < 2) return fail(F8_ERR_INVALID, "%s: block %d must be >= 2", fn, block);
    if (order != F8_ORDER_DCR && order != F8_ORDER_CRD) return fail(F8_ERR_INVALID, "%s: unknown order %d", fn, order);
    if (block > 16) return fail(F8_ERR_UNSUPPORTED, "%s: blocks above 16 are not built (got %d)", fn, block);
    const Tensor s = net->tensors[src];
    const int rr = block * block;
    if (!s2d && s.C % rr) return fail(F8_ERR_INVALID, "%s: the %d channels are no multiple of block^2 = %d", fn, s.C, rr);
    if (s2d && (s.H % block || s.W % block)) return fail(F8_ERR_INVALID, "%s: the %d x %d map is no multiple of block %d", fn, s.H, s.W, block);
    const int64_t C = s2d ? (int64_t)s.C * rr : s.C / rr, H = s2d ? s.H / block : (int64_t)s.H * block, W = s2d ? s.W / block : (int64_t)s.W * block;
    // the bound of f8_net_upsample on the map, and the result's padded int32 rows below 2 GiB an image
    if (H > INT32_MAX / 4 || W > INT32_MAX / 4 || H * W > INT32_MAX / 4 || C > INT32_MAX / 4 || H * W * ((C + 31) / 32 * 32) > INT32_MAX / 4)
        return fail(F8_ERR_UNSUPPORTED, "%s: the result [%lld, %lld, %lld] exceeds 2 GiB per tensor", fn, (long long)C, (long long)H, (long long)W);
    Node nd; nd.kind = s2d ? N_S2D : N_D2S; nd.a = src; nd.pm_block = block; nd.pm_order = order;
    net->nodes.push_back(nd);
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, (int)C, (int)H, (int)W, s.fl, id);
    net->nodes[id].out = t;
    net->tensors[src].consumers.push_back(id);
    return t;
}
int f8_net_depth_to_space(f8_net* net, int src, int block, int order) { return add_pixmap(net, src, block, order, false); }
int f8_net_space_to_depth(f8_net* net, int src, int block, int order) { return add_pixmap(net, src, block, order, true); }

int f8_net_mul(f8_net* net, int a, int b, const f8_mul_desc* desc) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_mul: null net");
    if (net->finalized) return fail(F8_ERR_STATE, "f8_net_mul: net already finalized");
    if (!desc) return fail(F8_ERR_INVALID, "f8_net_mul: null desc");
    if (const int rc = check_t(net, a, "f8_net_mul")) return rc;
    if (const int rc = check_t(net, b, "f8_net_mul")) return rc;
    const Tensor A = net->tensors[a], B = net->tensors[b];
    const bool same = B.C == A.C && B.H == A.H && B.W == A.W, gate = B.C == A.C && B.H == 1 && B.W == 1;
    if (!same && !gate)
        return fail(F8_ERR_INVALID, "f8_net_mul: b is [%d, %d, %d]: neither a's shape [%d, %d, %d] nor [%d, 1, 1]", B.C, B.H, B.W, A.C, A.H, A.W, A.C);
    // the operand formats are consumer formats: the conv's limits and shift range (consumer_format)
    f8_conv_desc fa{}, fb{};
    fa.input_fl = desc->a_fl; fa.input_signed = desc->a_signed != 0; fa.quant_input = 1;
    fb.input_fl = desc->b_fl; fb.input_signed = desc->b_signed != 0; fb.quant_input = 1;
    int n = 0;
    if (const int rc = consumer_format(A, fa, &n, "f8_net_mul (a)")) return rc;
    if (const int rc = consumer_format(B, fb, &n, "f8_net_mul (b)")) return rc;
    Node nd; nd.kind = N_MUL; nd.a = a; nd.b = b; nd.md = *desc;
    nd.md.a_signed = desc->a_signed != 0; nd.md.b_signed = desc->b_signed != 0; nd.md.relu = desc->relu != 0;
    net->nodes.push_back(nd);
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, A.C, A.H, A.W, desc->a_fl + desc->b_fl, id);
    net->nodes[id].out = t;
    net->tensors[a].consumers.push_back(id);
    net->tensors[b].consumers.push_back(id);      // (a == b: twice — two reads)
    return t;
}

int f8_net_hard_gate(f8_net* net, int src) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_hard_gate: null net");
    if (net->finalized) return fail(F8_ERR_STATE, "f8_net_hard_gate: net already finalized");
    if (const int rc = check_t(net, src, "f8_net_hard_gate")) return rc;
    const Tensor s = net->tensors[src];
    if (s.fl < 0 || s.fl > 28) return fail(F8_ERR_INVALID, "f8_net_hard_gate: source fraclen %d outside [0, 28] (6 * 2^fl must fit int32)", s.fl);
    Node nd; nd.kind = N_HGATE; nd.a = src;
    net->nodes.push_back(nd);
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, s.C, s.H, s.W, s.fl, id);
    net->nodes[id].out = t;
    net->tensors[src].consumers.push_back(id);
    return t;
}

int f8_net_table(f8_net* net, int src, const f8_table_desc* desc, const int32_t table_host[256]) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_table: null net");
    if (net->finalized) return fail(F8_ERR_STATE, "f8_net_table: net already finalized");
    if (!desc) return fail(F8_ERR_INVALID, "f8_net_table: null desc");
    if (!table_host) return fail(F8_ERR_INVALID, "f8_net_table: null table");
    if (const int rc = check_t(net, src, "f8_net_table")) return rc;
    const Tensor s = net->tensors[src];
    // the index format is a consumer format: the conv's limits and shift range (consumer_format)
    f8_conv_desc f{};
    f.input_fl = desc->in_fl; f.input_signed = desc->in_signed != 0; f.quant_input = 1;
    int n = 0;
    if (const int rc = consumer_format(s, f, &n, "f8_net_table")) return rc;
    if (desc->out_fl < 0 || desc->out_fl > 38)
        return fail(F8_ERR_INVALID, "f8_net_table: out_fl %d outside [0, 38] (beyond 38 no 8-bit format reads it: the shift would exceed 30)", desc->out_fl);
    Node nd; nd.kind = N_TABLE; nd.a = src; nd.td = *desc;
    nd.td.in_signed = desc->in_signed != 0;
    nd.table.assign(table_host, table_host + 256);
    net->nodes.push_back(std::move(nd));
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, s.C, s.H, s.W, desc->out_fl, id);
    net->nodes[id].out = t;
    net->tensors[src].consumers.push_back(id);
    return t;
}

int f8_net_maxpool(f8_net* net, int src, int k, int stride, int pad) {
    int rc = check_t(net, src, "f8_net_maxpool");
    if (rc) return rc;
    const Tensor& s = net->tensors[src];
    if (k < 1 || stride < 1 || pad < 0 || pad * 2 > k) return fail(F8_ERR_INVALID, "f8_net_maxpool: bad geometry");
    const int P = (s.H + 2 * pad - k) / stride + 1, Q = (s.W + 2 * pad - k) / stride + 1;
    if (P < 1 || Q < 1) return fail(F8_ERR_INVALID, "f8_net_maxpool: window larger than input");
    Node nd; nd.kind = N_MAXPOOL; nd.a = src; nd.pk = k; nd.pstride = stride; nd.ppad = pad;
    net->nodes.push_back(nd);
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, s.C, P, Q, s.fl, id);
    net->nodes[id].out = t;
    net->tensors[src].consumers.push_back(id);
    return t;
}

int f8_net_avgpool_sum(f8_net* net, int src, int shift) {
    int rc = check_t(net, src, "f8_net_avgpool_sum");
    if (rc) return rc;
    const Tensor& s = net->tensors[src];
    if (shift < 0 || s.fl + shift > 32)   // fix_quant_ops.py:129 `assert output_fraclen <= 32`
        return fail(F8_ERR_INVALID, "f8_net_avgpool_sum: output fraclen %d > 32", s.fl + shift);
    Node nd; nd.kind = N_AVGPOOL; nd.a = src; nd.shift = shift;
    net->nodes.push_back(nd);
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, s.C, 1, 1, s.fl + shift, id);
    net->nodes[id].out = t;
    net->tensors[src].consumers.push_back(id);
    return t;
}

int f8_net_avgpool_window(f8_net* net, int src, int kernel, int stride, int pad, int shift) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_avgpool_window: null net");
    if (net->finalized) return fail(F8_ERR_STATE, "f8_net_avgpool_window: net already finalized");
    if (const int rc = check_t(net, src, "f8_net_avgpool_window")) return rc;
    if (kernel < 1 || stride < 1 || pad < 0 || pad * 2 > kernel)
        return fail(F8_ERR_INVALID, "f8_net_avgpool_window: bad geometry (kernel %d, stride %d, pad %d: kernel, stride >= 1 and 0 <= 2 pad <= kernel)", kernel, stride, pad);
    if (kernel == 1 && stride == 1) return fail(F8_ERR_INVALID, "f8_net_avgpool_window: kernel 1 at stride 1 is the identity");
    if (kernel > 64 || stride > 64) return fail(F8_ERR_UNSUPPORTED, "f8_net_avgpool_window: kernels and strides above 64 are not built (got %d, %d)", kernel, stride);
    const Tensor s = net->tensors[src];
    if (s.H + 2 * pad < kernel || s.W + 2 * pad < kernel)
        return fail(F8_ERR_INVALID, "f8_net_avgpool_window: window %d larger than the padded %d x %d map", kernel, s.H + 2 * pad, s.W + 2 * pad);
    if (shift < 0) return fail(F8_ERR_INVALID, "f8_net_avgpool_window: shift %d < 0", shift);
    if (s.fl + shift > 32)   // fix_quant_ops.py:129 `assert output_fraclen <= 32`
        return fail(F8_ERR_INVALID, "f8_net_avgpool_window: output fraclen %d > 32", s.fl + shift);
    // the global window is not a new op: the node f8_net_avgpool_sum records, so it plans, fuses and names itself as before
    if (pad == 0 && kernel == s.H && kernel == s.W) return f8_net_avgpool_sum(net, src, shift);
    const int P = (s.H + 2 * pad - kernel) / stride + 1, Q = (s.W + 2 * pad - kernel) / stride + 1;
    Node nd; nd.kind = N_SUMPOOL; nd.a = src; nd.sum_k = kernel; nd.sum_stride = stride; nd.sum_pad = pad;
    net->nodes.push_back(nd);
    const int id = (int)net->nodes.size() - 1;
    const int t = new_tensor(net, s.C, P, Q, s.fl + shift, id);
    net->nodes[id].out = t;
    net->tensors[src].consumers.push_back(id);
    return t;
}

int f8_net_output(f8_net* net, int src, int as_float) {
    int rc = check_t(net, src, "f8_net_output");
    if (rc) return rc;
    if (output_index(net, src) >= 0) return fail(F8_ERR_INVALID, "f8_net_output: tensor %d is already output %d", src, output_index(net, src));
    if ((int)net->outs.size() >= F8_MAX_OUTPUTS) return fail(F8_ERR_UNSUPPORTED, "f8_net_output: at most %d outputs per net", F8_MAX_OUTPUTS);
    net->outs.push_back({src, as_float ? 1 : 0});
    return (int)net->outs.size() - 1;
}

int f8_net_output_argmax(f8_net* net, int src, int index_bytes) {
    int rc = check_t(net, src, "f8_net_output_argmax");
    if (rc) return rc;
    if (index_bytes != F8_IDX_U8 && index_bytes != F8_IDX_I32) return fail(F8_ERR_INVALID, "f8_net_output_argmax: index_bytes %d (F8_IDX_U8 or F8_IDX_I32)", index_bytes);
    const Tensor& s = net->tensors[src];
    if (s.C < 2) return fail(F8_ERR_INVALID, "f8_net_output_argmax: tensor %d has %d channel(s): the argmax needs at least 2", src, s.C);
    if (argmax_index(net, src) >= 0) return fail(F8_ERR_INVALID, "f8_net_output_argmax: tensor %d is already argmax output %d", src, argmax_index(net, src));
    if (index_bytes == F8_IDX_U8 && s.C > 255) return fail(F8_ERR_UNSUPPORTED, "f8_net_output_argmax: %d channels do not fit uint8 indices (255 is the poison value): use F8_IDX_I32", s.C);
    if ((int)net->outs.size() >= F8_MAX_OUTPUTS) return fail(F8_ERR_UNSUPPORTED, "f8_net_output_argmax: at most %d outputs per net", F8_MAX_OUTPUTS);
    net->outs.push_back({src, 0, index_bytes});
    return (int)net->outs.size() - 1;
}

int f8_net_output_kind(const f8_net* net, int k) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_output_kind: null net");
    if (k < 0 || k >= (int)net->outs.size()) return fail(F8_ERR_INVALID, "f8_net_output_kind: output %d of %d", k, (int)net->outs.size());
    const auto& o = net->outs[k];
    return o.idx == F8_IDX_U8 ? 2 : o.idx == F8_IDX_I32 ? 3 : o.as_float ? 1 : 0;
}

int f8_net_num_outputs(const f8_net* net) { return net ? (int)net->outs.size() : F8_ERR_INVALID; }

int f8_net_tensor_info(const f8_net* net, int t, int* C, int* H, int* W, int* fraclen) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_tensor_info: null net");
    if (t < 0 || t >= (int)net->tensors.size()) return fail(F8_ERR_INVALID, "f8_net_tensor_info: tensor %d of %d", t, (int)net->tensors.size());
    const Tensor& x = net->tensors[t];
    if (C) *C = x.C;
    if (H) *H = x.H;
    if (W) *W = x.W;
    if (fraclen) *fraclen = x.fl;
    return F8_OK;
}

int f8_net_output_info(const f8_net* net, int k, int* C, int* H, int* W, int* fraclen, int* as_float) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_output_info: null net");
    if (k < 0 || k >= (int)net->outs.size()) return fail(F8_ERR_INVALID, "f8_net_output_info: output %d of %d", k, (int)net->outs.size());
    const Tensor& t = net->tensors[net->outs[k].t];
    const bool amax = net->outs[k].idx != 0;           // a class map: one channel of indices, no fraclen
    if (C) *C = amax ? 1 : t.C;
    if (H) *H = t.H;
    if (W) *W = t.W;
    if (fraclen) *fraclen = amax ? 0 : t.fl;
    if (as_float) *as_float = net->outs[k].as_float;
    return F8_OK;
}

int f8_net_set_output_buffers(f8_net* net, void* const* bufs_dev, int n) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_set_output_buffers: null net");
    if (!net->finalized) return fail(F8_ERR_STATE, "f8_net_set_output_buffers: not finalized");
    if (n != (int)net->outs.size() - 1) return fail(F8_ERR_INVALID, "f8_net_set_output_buffers: %d buffers for outputs 1 .. %d", n, (int)net->outs.size() - 1);
    for (int k = 0; k < n; ++k) if (!bufs_dev || !bufs_dev[k]) return fail(F8_ERR_INVALID, "f8_net_set_output_buffers: null pointer");
    for (int k = 0; k < n; ++k) net->out_bufs[k] = bufs_dev[k];
    net->out_bufs_set = true;
    return F8_OK;
}

int f8_net_set_pipelined(f8_net* net, int on) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_set_pipelined: null net");
    net->pipelined = on == 2 ? 2 : (on ? 1 : 0);
    net->pipe_count = 0;
    return F8_OK;
}

int f8_net_set_label(f8_net* net, int t, const char* label) {
    if (!net || t < 0 || t >= (int)net->tensors.size()) return fail(F8_ERR_INVALID, "f8_net_set_label: bad tensor");
    net->tensors[t].label = label ? label : "";
    return F8_OK;
}

// ------------------------------------------------------------------------------ planner
static void pack_conv_bias(f8_net* net, Node& nd, const std::vector<long long>& tapsum);
static void pack_conv_weights(f8_net* net, Node& nd) {
    // Packed layout: [coutP][taps][CK] int8, K-contiguous per output channel, zero padded.
    // Generic: tap = (r,s), CK = Cs(src) channels.  Stem (cin <= 4, source = network input held as
    // haloed NHWC4): one "tap" per kernel ROW, CK = 32 bytes = 8 pixels x 4 channels of which
    // the first kw pixels / cin channels carry weights.
    // Bias: unsigned inputs are stored biased (x - 128), so b' = b + 128 * sum of w over the taps that
    // lie INSIDE the image.  Zero padding is fetched as biased 0 (= real 128) and must not be
    // corrected for taps outside; which taps are outside depends only on the output row / column, so
    // rows and columns are classified by their in-image tap mask and the table is
    // bias[rowclass * ncc + colclass][cout].  Signed inputs / unpadded convs have one class.
    // A grouped conv (the dense expansion): raw weights [cout][cin / groups][k][k]; output channel o reads the input channels of ITS group only, every
    // other weight of its row stays zero (block-diagonal), and its tap sums run over those cin / groups weights.
    const f8_conv_desc& d = nd.cd;
    const Tensor& src = net->tensors[nd.a];
    const f8_conv_geom g = geom_of(nd);
    const int kh = g.kh, kw = g.kw;              // (a rectangular conv: taps (r, s) of kh rows x kw columns, [coutP][(r * kw + s) * Cs + c]; never the stem)
    const int cg = d.cin / d.groups, kg = d.cout / d.groups;
    nd.coutP = round_up(d.cout, 32);
    if (nd.stem) { nd.ck = 32; nd.ktot = kh * 32; }
    else { nd.ck = src.Cs; nd.ktot = kh * kw * src.Cs; }
    nd.w_off = round_up_z(net->wblob.size(), 256);
    const size_t wbytes = (size_t)nd.coutP * nd.ktot;
    net->wblob.resize(nd.w_off + wbytes, 0);
    // per-tap weight sums
    std::vector<long long> tapsum((size_t)d.cout * kh * kw, 0);
    {
        int8_t* wp = (int8_t*)net->wblob.data() + nd.w_off;
        for (int o = 0; o < d.cout; ++o)
            for (int ci = 0; ci < cg; ++ci)
                for (int r = 0; r < kh; ++r)
                    for (int s = 0; s < kw; ++s) {
                        const int8_t v = nd.w[(((size_t)o * cg + ci) * kh + r) * kw + s];
                        const int c = (o / kg) * cg + ci;       // the input channel (groups == 1: ci)
                        tapsum[((size_t)o * kh + r) * kw + s] += v;
                        size_t idx;
                        if (nd.stem) idx = (size_t)o * nd.ktot + (size_t)r * 32 + (size_t)s * 4 + c;
                        else idx = (size_t)o * nd.ktot + ((size_t)(r * kw + s)) * src.Cs + c;
                        wp[idx] = v;
                    }
    }
    pack_conv_bias(net, nd, tapsum);
}

// The border-class bias table of a conv whose weights are packed (nd.coutP set): bias[rowclass * ncc + colclass][coutP] and the class of every output
// row / column (pack_conv_weights); tapsum[cout][kh][kw] = the sum over the input channels of each tap's weights.  Each axis is classified with its own
// kernel size, stride and LEADING pad (geom_of); a trailing pad shows only in the number of outputs and in which of them lose taps.
static void pack_conv_bias(f8_net* net, Node& nd, const std::vector<long long>& tapsum) {
    const f8_conv_desc& d = nd.cd;
    const Tensor& src = net->tensors[nd.a]; const Tensor& dst = net->tensors[nd.out];
    const f8_conv_geom g = geom_of(nd);
    const int kh = g.kh, kw = g.kw;
    // classes
    std::vector<uint32_t> rmasks, cmasks;
    std::vector<uint8_t> rowcls(dst.H, 0), colcls(dst.W, 0);
    const bool classes = !d.input_signed && (g.pad_top > 0 || g.pad_left > 0 || g.pad_bottom > 0 || g.pad_right > 0) && !nd.stem && !nd.no_classes;
    if (classes) {
        auto classify = [&](int n_out, int n_in, int k, int stride, int pad, std::vector<uint32_t>& masks, std::vector<uint8_t>& cls) {
            for (int p = 0; p < n_out; ++p) {
                uint32_t mk = 0;
                for (int r = 0; r < k; ++r) { const int h = p * stride - pad + r * nd.dil; if (h >= 0 && h < n_in) mk |= 1u << r; }
                size_t id = 0;
                while (id < masks.size() && masks[id] != mk) ++id;
                if (id == masks.size()) masks.push_back(mk);
                cls[p] = (uint8_t)id;
            }
        };
        classify(dst.H, src.H, kh, g.stride_h, g.pad_top, rmasks, rowcls);
        classify(dst.W, src.W, kw, g.stride_w, g.pad_left, cmasks, colcls);
    } else {
        rmasks.push_back((1u << kh) - 1); cmasks.push_back((1u << kw) - 1);
    }
    nd.ncc = classes ? (int)cmasks.size() : 0;
    const size_t ncls = rmasks.size() * cmasks.size();
    nd.b_off = round_up_z(net->wblob.size(), 256);
    net->wblob.resize(nd.b_off + ncls * (size_t)nd.coutP * 4, 0);
    int32_t* bp = (int32_t*)(net->wblob.data() + nd.b_off);
    for (size_t rc = 0; rc < rmasks.size(); ++rc)
        for (size_t cc = 0; cc < cmasks.size(); ++cc)
            for (int o = 0; o < d.cout; ++o) {
                long long sum = 0;
                for (int r = 0; r < kh; ++r)
                    for (int s = 0; s < kw; ++s)
                        if (((rmasks[rc] >> r) & 1u) && ((cmasks[cc] >> s) & 1u)) sum += tapsum[((size_t)o * kh + r) * kw + s];
                uint32_t b = (uint32_t)nd.bias[o];
                if (!d.input_signed) b += (uint32_t)(128ll * sum);
                bp[(rc * cmasks.size() + cc) * (size_t)nd.coutP + o] = (int32_t)b;
            }
    if (classes) {
        nd.rc_off = round_up_z(net->wblob.size(), 256);
        net->wblob.resize(nd.rc_off + rowcls.size(), 0);
        memcpy(net->wblob.data() + nd.rc_off, rowcls.data(), rowcls.size());
        nd.cc_off = round_up_z(net->wblob.size(), 256);
        net->wblob.resize(nd.cc_off + colcls.size(), 0);
        memcpy(net->wblob.data() + nd.cc_off, colcls.data(), colcls.size());
    }
}

// A transposed conv's weights, biases and phase table.  Output phase (rh, rw) = ((oh + pad) % s, (ow + pad) % s) sees the kernel rows
// kh = rh + s th, th < Th = ceil((k - rh) / s) — none where k <= rh — at the input row ih = a - th, oh = s a + rh - pad; its weights are one plain
// GEMM operand [coutP][Th * Tw * CK], K = (th * Tw + tw) * CK + ci, stored in MFMA-fragment order (as pack_frag_weights: [cout tile of 32][K32 step]
// [lane 0..63][16 B], lane l = row l & 31 of the tile, bytes [32 step + 16 (l >> 5), +16): one coalesced 1 KB per wave load), the phases one behind
// the other from Node::w_off (DeconvPhase::w_off is relative to it; Node::ktot = the bytes per output channel summed over the phases = k * k * CK).
// Bias: the border-class table of pack_conv_bias with the transposed conv's rule — the class of an OUTPUT row oh is the set of kernel rows kh with
// oh + pad - kh = s ih for an in-image ih, and bias[rowclass * ncc + colclass][co] = b + 128 * (sum of w over that set x the column's set) for unsigned
// (biased) inputs; an empty set leaves the bias alone.  Rows near either border miss taps even at pad 0, so unsigned inputs always have classes.
static void pack_deconv_weights(f8_net* net, Node& nd) {
    const f8_conv_desc& d = nd.cd;
    const Tensor& src = net->tensors[nd.a]; const Tensor& dst = net->tensors[nd.out];
    const int k = d.kernel, s = d.stride, CK = src.Cs;
    nd.coutP = round_up(d.cout, 32);
    nd.ck = CK; nd.ktot = k * k * CK;
    nd.w_off = round_up_z(net->wblob.size(), 256);
    net->wblob.resize(nd.w_off + (size_t)nd.coutP * nd.ktot, 0);
    auto wraw = [&](int ci, int co, int r, int c) { return nd.w[(((size_t)ci * d.cout + co) * k + r) * k + c]; };
    size_t off = 0;
    for (int rh = 0; rh < s; ++rh)
        for (int rw = 0; rw < s; ++rw) {
            DeconvPhase& p = nd.dph[rh * s + rw];
            p = DeconvPhase{};
            p.rh = rh; p.rw = rw;
            p.Th = rh < k ? (k - rh + s - 1) / s : 0; p.Tw = rw < k ? (k - rw + s - 1) / s : 0;
            // the sub-grid: a >= a0 is the first index with oh = s a + rh - pad >= 0, and A of them stay below the output's height
            auto grid = [&](int r, int n_out, int32_t* first, int32_t* count) {
                *first = d.pad > r ? (d.pad - r + s - 1) / s : 0;
                const int last = n_out - 1 + d.pad - r >= 0 ? (n_out - 1 + d.pad - r) / s : -1;
                *count = std::max(0, last - *first + 1);
            };
            grid(rh, dst.H, &p.a0, &p.A);
            grid(rw, dst.W, &p.c0, &p.Cn);
            p.dAC = fast_divisor((uint32_t)std::max(1, p.A * p.Cn));
            p.dC = fast_divisor((uint32_t)std::max(1, p.Cn));
            p.w_off = (uint32_t)off;
            const size_t kp = (size_t)p.Th * p.Tw * CK;
            int8_t* wp = (int8_t*)net->wblob.data() + nd.w_off + off;
            for (int co = 0; co < d.cout; ++co)
                for (int th = 0; th < p.Th; ++th)
                    for (int tw = 0; tw < p.Tw; ++tw)
                        for (int ci = 0; ci < d.cin; ++ci) {
                            const size_t kidx = ((size_t)th * p.Tw + tw) * CK + ci, nk = kp / 32;      // K32 step kidx / 32, lane half (kidx % 32) / 16
                            wp[((((size_t)(co >> 5) * nk + kidx / 32) * 64) + ((kidx % 32) / 16) * 32 + (co & 31)) * 16 + kidx % 16] = wraw(ci, co, rh + s * th, rw + s * tw);
                        }
            off += (size_t)nd.coutP * kp;
        }
    // per-tap weight sums and the class tables
    std::vector<long long> tapsum((size_t)d.cout * k * k, 0);
    for (int ci = 0; ci < d.cin; ++ci)
        for (int co = 0; co < d.cout; ++co)
            for (int r = 0; r < k; ++r)
                for (int c = 0; c < k; ++c) tapsum[((size_t)co * k + r) * k + c] += wraw(ci, co, r, c);
    std::vector<uint32_t> rmasks, cmasks;
    std::vector<uint8_t> rowcls(dst.H, 0), colcls(dst.W, 0);
    const bool classes = !d.input_signed;
    if (classes) {
        auto classify = [&](int n_out, int n_in, std::vector<uint32_t>& masks, std::vector<uint8_t>& cls) {
            for (int o = 0; o < n_out; ++o) {
                uint32_t mk = 0;
                for (int r = 0; r < k; ++r) { const int v = o + d.pad - r; if (v >= 0 && v % s == 0 && v / s < n_in) mk |= 1u << r; }
                size_t id = 0;
                while (id < masks.size() && masks[id] != mk) ++id;
                if (id == masks.size()) masks.push_back(mk);
                cls[o] = (uint8_t)id;
            }
        };
        classify(dst.H, src.H, rmasks, rowcls);
        classify(dst.W, src.W, cmasks, colcls);
    } else {
        rmasks.push_back(0); cmasks.push_back(0);                   // signed inputs: zero is zero, the bias is the bias
    }
    nd.ncc = classes ? (int)cmasks.size() : 0;
    nd.b_off = round_up_z(net->wblob.size(), 256);
    net->wblob.resize(nd.b_off + rmasks.size() * cmasks.size() * (size_t)nd.coutP * 4, 0);
    int32_t* bp = (int32_t*)(net->wblob.data() + nd.b_off);
    for (size_t rc = 0; rc < rmasks.size(); ++rc)
        for (size_t cc = 0; cc < cmasks.size(); ++cc)
            for (int o = 0; o < d.cout; ++o) {
                long long sum = 0;
                for (int r = 0; r < k; ++r)
                    for (int c = 0; c < k; ++c)
                        if (((rmasks[rc] >> r) & 1u) && ((cmasks[cc] >> c) & 1u)) sum += tapsum[((size_t)o * k + r) * k + c];
                bp[(rc * cmasks.size() + cc) * (size_t)nd.coutP + o] = (int32_t)((uint32_t)nd.bias[o] + (uint32_t)(128ll * sum));
            }
    if (classes) {
        nd.rc_off = round_up_z(net->wblob.size(), 256);
        net->wblob.resize(nd.rc_off + rowcls.size(), 0);
        memcpy(net->wblob.data() + nd.rc_off, rowcls.data(), rowcls.size());
        nd.cc_off = round_up_z(net->wblob.size(), 256);
        net->wblob.resize(nd.cc_off + colcls.size(), 0);
        memcpy(net->wblob.data() + nd.cc_off, colcls.data(), colcls.size());
    }
}

// A second image of a conv's packed weights ([coutP][ktot], K-contiguous) in MFMA-fragment order:
//   [cout tile of 32][K32 step][lane 0..63][16 B],  lane l = row (l & 31) of the tile, bytes [32 * step + 16 * (l >> 5), +16)
// — the A operand of one v_mfma_i32_32x32x32_i8 is one contiguous 1 KB, so a wave fetches it with one coalesced instruction straight
// into registers (f8_p12.hip: no LDS staging, no barrier in the K loop).
static void pack_frag_weights(f8_net* net, Node& nd) {
    const size_t bytes = (size_t)nd.coutP * nd.ktot;
    nd.wf_off = round_up_z(net->wblob.size(), 256);
    net->wblob.resize(nd.wf_off + bytes, 0);
    const int8_t* src = (const int8_t*)net->wblob.data() + nd.w_off;
    int8_t* dst = (int8_t*)net->wblob.data() + nd.wf_off;
    const int steps = nd.ktot / 32;
    for (int t = 0; t < nd.coutP / 32; ++t)
        for (int s = 0; s < steps; ++s)
            for (int l = 0; l < 64; ++l)
                memcpy(dst + (((size_t)t * steps + s) * 64 + l) * 16, src + (size_t)(t * 32 + (l & 31)) * nd.ktot + s * 32 + (l >> 5) * 16, 16);
}

static void pack_dw_weights(f8_net* net, Node& nd) {
    // Two images of the depthwise weights:
    //  (1) [9][Cs] tap-major + plain bias            — scalar kernel (int32 outputs, fallback)
    //  (2) [Cs/4][9] dwords for the dot4 kernel: per 4-channel quad, dword e (0..3) = taps 0..3 of channel e,
    //      dword 4+e = taps 4..7 of channel e, dword 8 = tap 8 of the 4 channels; bias + 128 * sum(w) when the
    //      input is unsigned (stored biased; out-of-image taps are replaced by the biased zero in the kernel).
    const f8_conv_desc& d = nd.cd;
    const Tensor& src = net->tensors[nd.a];
    nd.coutP = src.Cs; nd.ck = 0; nd.ktot = 0;
    nd.w_off = round_up_z(net->wblob.size(), 256);
    nd.b_off = round_up_z(nd.w_off + (size_t)9 * src.Cs, 256);
    nd.rc_off = round_up_z(nd.b_off + (size_t)src.Cs * 4, 256);            // dot4 weights
    nd.cc_off = round_up_z(nd.rc_off + (size_t)(src.Cs / 4) * 9 * 4, 256);  // dot4 bias
    net->wblob.resize(nd.cc_off + (size_t)src.Cs * 4, 0);
    int8_t* wp = (int8_t*)net->wblob.data() + nd.w_off;
    int32_t* bp = (int32_t*)(net->wblob.data() + nd.b_off);
    int8_t* w4 = (int8_t*)net->wblob.data() + nd.rc_off;
    int32_t* b4 = (int32_t*)(net->wblob.data() + nd.cc_off);
    for (int c = 0; c < d.cout; ++c) {
        long long sum = 0;
        for (int t = 0; t < 9; ++t) {
            const int8_t v = nd.w[(size_t)c * 9 + t];
            wp[(size_t)t * src.Cs + c] = v;
            sum += v;
            int8_t* quad = w4 + (size_t)(c / 4) * 36;
            const int e = c % 4;
            if (t < 4) quad[e * 4 + t] = v;
            else if (t < 8) quad[16 + e * 4 + (t - 4)] = v;
            else quad[32 + e] = v;
        }
        bp[c] = nd.bias[c];
        uint32_t b = (uint32_t)nd.bias[c];
        if (!d.input_signed) b += (uint32_t)(128ll * sum);
        b4[c] = (int32_t)b;
    }
}

// "General depthwise": every accepted depthwise conv that is not 3x3 / pad 1 (kernel 3 / 5 / 7, stride 1 / 2, pad 0 .. kernel / 2; add_conv_node).  One pass
// of the planner fuses one — 1e3, option fuse_irk: kernel 5 / 7 with pad kernel / 2 inside an inverted residual —; every other matcher asks for kernel 3
// and pad 1, so anywhere else it is a launch of its own on the kernels of f8_dwk.hip.
static bool dw_general(const Node& n) { const f8_conv_desc& d = n.cd; return d.groups != 1 && d.groups == d.cin && !(d.kernel == 3 && d.pad == 1 && n.dil == 1); }

// The two weight images of a general depthwise conv, at offsets of their own (the 3x3 / pad 1 images are pack_dw_weights' and stay as they are):
//  (1) [K * K][Cs] tap-major + plain bias                        — dwconvk_kernel
//  (2) [Cs / 4][K columns][G = ceil(K / 4) row groups][4 channels] dwords for dwconvk_dot4_kernel: byte j of dword (quad, s, g, e) = the weight of
//      channel 4 * quad + e at row 4 g + j, column s — 0 for the rows beyond K, whose slots of a dot4 may then hold any byte; bias + 128 * sum(w)
//      when the input is unsigned (stored biased; the kernel replaces out-of-image taps by the biased zero).
static void pack_dwk_weights(f8_net* net, Node& nd) {
    const f8_conv_desc& d = nd.cd;
    const Tensor& src = net->tensors[nd.a];
    const f8_conv_geom g = geom_of(nd);
    const int KH = g.kh, KW = g.kw, K = std::max(KH, KW), G = (K + 3) / 4;
    // a strip (f8_net_conv_rect: 1 x K or K x 1): image (1) is [KH * KW][Cs]; image (2) is dwstrip_dot4_kernel's — [Cs / 4][4 phases][NW = ceil((K + 3) / 4)]
    // [4 channels] dwords, byte b of dword (quad, ph, m, e) = tap 4 m + b - ph of channel 4 quad + e, 0 outside 0 .. K - 1: the K taps shifted by ph bytes
    const int NW = (K + 3 + 3) / 4;
    const size_t w4_bytes = nd.rect ? (size_t)(src.Cs / 4) * 4 * NW * 16 : (size_t)(src.Cs / 4) * K * G * 16;
    nd.coutP = src.Cs; nd.ck = 0; nd.ktot = 0;
    nd.w_off = round_up_z(net->wblob.size(), 256);
    nd.b_off = round_up_z(nd.w_off + (size_t)KH * KW * src.Cs, 256);
    nd.rc_off = round_up_z(nd.b_off + (size_t)src.Cs * 4, 256);                    // dot4 weights
    nd.cc_off = round_up_z(nd.rc_off + w4_bytes, 256);                             // dot4 bias
    net->wblob.resize(nd.cc_off + (size_t)src.Cs * 4, 0);
    int8_t* wp = (int8_t*)net->wblob.data() + nd.w_off;
    int32_t* bp = (int32_t*)(net->wblob.data() + nd.b_off);
    int8_t* w4 = (int8_t*)net->wblob.data() + nd.rc_off;
    int32_t* b4 = (int32_t*)(net->wblob.data() + nd.cc_off);
    for (int c = 0; c < d.cout; ++c) {
        long long sum = 0;
        for (int r = 0; r < KH; ++r)
            for (int s = 0; s < KW; ++s) {
                const int8_t v = nd.w[((size_t)c * KH + r) * KW + s];
                wp[(size_t)(r * KW + s) * src.Cs + c] = v;
                sum += v;
                if (!nd.rect) { w4[((((size_t)(c / 4) * K + s) * G + r / 4) * 4 + c % 4) * 4 + r % 4] = v; continue; }
                const int t = r + s;                            // the tap along the strip (one of r, s is 0)
                for (int ph = 0; ph < 4; ++ph)
                    w4[((((size_t)(c / 4) * 4 + ph) * NW + (t + ph) / 4) * 4 + c % 4) * 4 + (t + ph) % 4] = v;
            }
        bp[c] = nd.bias[c];
        uint32_t b = (uint32_t)nd.bias[c];
        if (!d.input_signed) b += (uint32_t)(128ll * sum);
        b4[c] = (int32_t)b;
    }
}

// A grouped 3x3 on gconv3x3_kernel (f8_gconv.hip; gconv_kernel_applies: cin == cout, cg = cin / groups divides 32): per 32-channel slice t and tap, the
// 32 x 32 block W[cout 32 t + i][cin 32 t + j] — zero wherever the two channels are not of one group, or beyond C — in MFMA-fragment order
// [slice][tap][lane][16 B]: lane l = row (l & 31), input channels 32 t + 16 (l >> 5) .. + 15.  The bias table is pack_conv_weights' (the tap sums run over
// the cg weights of the group).
static void pack_gconv_weights(f8_net* net, Node& nd) {
    const f8_conv_desc& d = nd.cd;
    const Tensor& src = net->tensors[nd.a];
    const int cg = d.cin / d.groups, nsl = src.Cs / 32;
    nd.coutP = src.Cs; nd.ck = 32; nd.ktot = 9 * 32;
    nd.w_off = round_up_z(net->wblob.size(), 256);
    net->wblob.resize(nd.w_off + (size_t)nsl * 9 * 1024, 0);
    std::vector<long long> tapsum((size_t)d.cout * 9, 0);
    int8_t* wp = (int8_t*)net->wblob.data() + nd.w_off;
    for (int o = 0; o < d.cout; ++o)
        for (int ci = 0; ci < cg; ++ci) {
            const int c = (o / cg) * cg + ci;                   // input channel: same group, hence same slice (cg divides 32)
            const int lane = (o & 31) + 32 * ((c & 31) >> 4);
            for (int t = 0; t < 9; ++t) {
                const int8_t v = nd.w[((size_t)o * cg + ci) * 9 + t];
                tapsum[(size_t)o * 9 + t] += v;
                wp[(((size_t)(o >> 5) * 9 + t) * 64 + lane) * 16 + (c & 15)] = v;
            }
        }
    pack_conv_bias(net, nd, tapsum);
}

static std::string tname(const f8_net* net, int t) {
    const Tensor& T = net->tensors[t];
    if (!T.label.empty()) return T.label;
    char b[32]; snprintf(b, sizeof b, "t%d", t);
    return b;
}

// choose the forms a producer writes; extra int8 formats beyond two need the int32 form
static void select_outputs(f8_net* net, int t, OutSel* o, std::vector<int>* extra) {
    Tensor& T = net->tensors[t];
    o->t = t;
    int n8 = 0;
    for (size_t i = 0; i < T.forms.size(); ++i) if (T.forms[i].kind == FORM_I8) ++n8;
    if (n8 > 2) add_form(T, FORM_I32, 0, 0);
    o->f32 = find_form(T, FORM_I32, 0, 0);
    int k = 0;
    for (size_t i = 0; i < T.forms.size(); ++i)
        if (T.forms[i].kind == FORM_I8) {
            if (k < 2) o->f8[k++] = (int)i;
            else if (extra) extra->push_back((int)i);
        }
}
// ... for a launch of its own whose result nothing asked for in any form: it writes the int32 form
static void select_outputs_or_i32(f8_net* net, int t, OutSel* o, std::vector<int>* extra) {
    if (net->tensors[t].forms.empty()) add_form(net->tensors[t], FORM_I32, 0, 0);
    select_outputs(net, t, o, extra);
}

// Essential vector work of a launch (VERDICT r5 #1b: the counters' SQ_INSTS_VALU x 64 divided by this = issued / essential): per value of the
// reference's semantics, with the cheapest exact integer forms of f8_device.h —
//   an int8 value produced (in HBM or only in LDS): round-half-even shift + clamp + pack = 3 (v_bfe_u32, v_add3_u32, 1/2 v_ashr_pk_u8_i32, 1/4 v_perm_b32,
//   1/4 v_xor_b32; the ReLU in front of it is the clamp's lower bound); a joined int32 value: align-add + clamp / ReLU = 2; a max-pooled conv value: 1.
// Addressing, lane swaps, exec masks, halo code, tile padding and recompute are NOT in it: they are what the ratio shows.
static double out_forms8(const Step& st) { return (double)((st.out.f8[0] >= 0) + (st.out.f8[1] >= 0)); }
static bool only_stem_form(const Tensor& o) {           // the network input's one form is the stem's haloed NHWC4 copy
    bool only = !o.forms.empty();
    for (auto& F : o.forms) only = only && F.kind == FORM_STEM;
    return only;
}
// Name of a conv step: the kernel (its variant; the tile of conv_igemm) + the layer key.  (The device symbol, Step::kernel: bind_step.)
static void label_conv_step(f8_net* net, Step& st, const Node& nd) {
    const f8_conv_desc& d = nd.cd;
    const bool res = st.res_t >= 0;
    const std::string key = nd.dual >= 0 ? tname(net, net->nodes[nd.dual].out) + "+" + tname(net, nd.out) : tname(net, nd.out);
    char buf[160], dl[16] = "";                  // d<D> behind the stride of a dilated conv
    if (nd.dil > 1) snprintf(dl, sizeof dl, "d%d", nd.dil);
    if (nd.rect) {                               // conv1x7s1_..., conv3x5s2x1_... where the strides differ; dwconv1x21s1:
        const f8_conv_geom& g = nd.rg;
        char ss[24];
        if (g.stride_h == g.stride_w) snprintf(ss, sizeof ss, "%d", g.stride_h); else snprintf(ss, sizeof ss, "%dx%d", g.stride_h, g.stride_w);
        if (nd.depthwise) snprintf(buf, sizeof buf, "dwconv%dx%ds%s:%s", g.kh, g.kw, ss, key.c_str());
        else snprintf(buf, sizeof buf, "conv%dx%ds%s%s_t%dx%dx%d%s:%s", g.kh, g.kw, ss, dl, nd.tile.bm, nd.tile.bn, nd.tile.bk, res ? "_res" : "", key.c_str());
        st.name = buf;
        return;
    }
    switch (st.variant) {
        case V_FC: st.name = "linear_dense:" + key; return;
        case V_POOL: st.name = (res ? "conv1x1_res+avgpool:" : "conv1x1+avgpool:") + key; return;
        case V_WSTAT: st.name = (nd.dual >= 0 ? "conv1x1_wstat_dual:" : res ? "conv1x1_wstat_res:" : "conv1x1_wstat:") + key; return;
        case V_S2WREG: st.name = "conv3x3s2_wreg:" + key; return;
        case V_WREG: st.name = "conv1x1s1_wreg:" + key; return;
        case V_PATCH3X3: snprintf(buf, sizeof buf, "conv3x3s1_patch_R%dx%d_bn%d%s:%s", nd.p3_R, nd.p3_imgs, nd.p3_bn, res ? "_res" : "", key.c_str()); break;
        default:
            if (nd.depthwise) snprintf(buf, sizeof buf, "dwconv%dx%ds%d%s:%s", d.kernel, d.kernel, d.stride, dl, key.c_str());
            else if (nd.grouped) snprintf(buf, sizeof buf, "gconv%dx%ds%d%s_dense:%s", d.kernel, d.kernel, d.stride, dl, key.c_str());
            else snprintf(buf, sizeof buf, "conv%dx%ds%d%s_t%dx%dx%d%s%s:%s", d.kernel, d.kernel, d.stride, dl, nd.tile.bm, nd.tile.bn,
                          nd.tile.bk, nd.stem ? "_stem" : "", res ? "_res" : (nd.dual >= 0 ? "_dual" : ""), key.c_str());
    }
    st.name = buf;
}

// ================================================================================================================================
// The planner: f8_net_finalize runs these passes in order.  Passes 1 .. 1i only record which launch runs which conv — one Block per
// fused block on its host conv (set_block), chain membership (set_chain), the pairwise links fused_add / dual / pool —;
// pass 2 decides the forms each tensor needs in HBM, pass 3 emits the launches, pass 4 lays the arena out.  Round 5: one function per pass
// (round 4: one 1100-line function).
// ================================================================================================================================

// position of a block (by its host conv) inside its chain launch, -1: not chained
static int chain_pos(const f8_net* net, int host) {
    const auto& ND = net->nodes;
    if (host < 0 || ND[host].chain_into < 0) return -1;
    const std::vector<int>& ch = ND[ND[host].chain_into].chain;
    for (size_t k = 0; k < ch.size(); ++k) if (ch[k] == host) return (int)k;
    return -1;
}
// the blocks hosted by `hosts`, in order, become one chain launch
static void set_chain(f8_net* net, const std::vector<int>& hosts, ChainKind kind) {
    Node& last = net->nodes[hosts.back()];
    for (int h : hosts) net->nodes[h].chain_into = hosts.back();
    last.chain = hosts; last.chain_kind = kind;
}
// Conv `host` becomes the host of block B and B's other convs its members.  The record's invariant — a conv hosts at most one block and is a member
// of at most one — is checked here, once per block of every finalize: a pass that takes over what an earlier one marked releases it first.
static void set_block(f8_net* net, int host, const Block& B) {
    auto& ND = net->nodes;
    if (ND[host].blk.kind != B_NONE && net->plan_bug < 0) net->plan_bug = host;
    ND[host].blk = B;
    for (int c : {B.b0, B.b2, B.b4, B.sc}) {
        if (c < 0 || c == host || c == ND[host].dual) continue;      // (the other conv of the host's dual GEMM is linked by dual / dual_host)
        if ((ND[c].absorbed_by >= 0 || ND[c].blk.kind != B_NONE) && net->plan_bug < 0) net->plan_bug = c;
        ND[c].absorbed_by = host;
    }
}
// ... and stops being one: its members are convs of their own again
static void release_block(f8_net* net, int host) {
    auto& ND = net->nodes;
    const Block B = ND[host].blk;
    for (int c : {B.b0, B.b2, B.b4, B.sc})
        if (c >= 0 && ND[c].absorbed_by == host) { ND[c].absorbed_by = -1; ND[c].no_classes = false; }
    ND[host].blk = Block{};
}
// Is conv i taken by a fused launch: does it host a block, is it a member of one, or is it in a chain?  (Hosting a dual GEMM — Node::dual — is
// not in it: the stage-opening blocks are built on that link.)  `but`: hosting a block of that kind does not count, for a pass that takes over
// what an earlier one marked.
static bool claimed(const f8_net* net, int i, BlockKind but = B_NONE) {
    const Node& n = net->nodes[i];
    return n.absorbed_by >= 0 || n.dual_host >= 0 || n.chain_into >= 0 || (n.blk.kind != B_NONE && n.blk.kind != but);
}
// The role conv i plays in a fused block, and in whose (*host); R_NONE: in none
static Role role_in_block(const f8_net* net, int i, int* host) {
    const Node& n = net->nodes[i];
    const int h = n.blk.kind != B_NONE ? i : (n.absorbed_by >= 0 ? n.absorbed_by : n.dual_host);
    if (h < 0) return R_NONE;
    const Block& B = net->nodes[h].blk;
    const Role r = B.b0 == i ? R_B0 : B.b2 == i ? R_B2 : B.b4 == i ? R_B4 : B.sc == i ? R_SC : R_NONE;
    if (r != R_NONE) *host = h;
    return r;
}

// ---- The vocabulary of the matchers (passes 1 .. 1k).  What the passes really differ in — quant_input, relu, fused_add, dual, claimed() — stays
// written out where a pass tests it.  Every tensor has a producer (f8_net_input, add_conv_node and the other builders create it with one): no pass tests for that.
// a plain conv (groups 1) of this kernel, stride and pad, undilated: a dilated conv joins no fused launch
static bool plain_conv(const Node& n, int k, int s, int p) {
    return n.kind == N_CONV && n.cd.groups == 1 && n.cd.kernel == k && n.dil == 1 && n.cd.stride == s && n.cd.pad == p;
}
// a depthwise conv (groups == cin, more than one channel; add_conv_node then insists on cout == cin) of this kernel and pad, stride 1 (stride2: or 2)
static bool depthwise_conv(const Node& n, int k, int p, bool stride2) {
    return n.kind == N_CONV && n.cd.groups != 1 && n.cd.groups == n.cd.cin && n.cd.kernel == k && n.dil == 1 && n.cd.pad == p &&
           (n.cd.stride == 1 || (stride2 && n.cd.stride == 2));
}
// tensor t as a private intermediate: its producer node if exactly one node reads it and it is no network output, else -1
static int private_producer(const f8_net* net, int t) {
    const Tensor& x = net->tensors[t];
    return x.consumers.size() == 1 && !is_output(net, t) ? x.prod : -1;
}
// conv c hosts a residual join (c.fused_add >= 0): the tensor on the join's other side
static int join_other(const f8_net* net, const Node& c) {
    const Node& ad = net->nodes[c.fused_add];
    return ad.a == c.out ? ad.b : ad.a;
}
// Can a launch that writes int8 forms only produce tensor t (passes 1j / 1k): is every reader a conv of its own — or the member of a depthwise-separable
// block — that requantises its input, in at most two formats between them?
static bool int8_readers_only(const f8_net* net, int t) {
    const auto& ND = net->nodes;
    std::vector<std::pair<int, int>> fmts;
    for (int u : net->tensors[t].consumers) {
        const Node& un = ND[u];
        int n = 0;
        if ((un.kind != N_CONV && un.kind != N_LINEAR) || !un.cd.quant_input || consumer_format(net->tensors[t], un.cd, &n, "finalize") ||
            (claimed(net, u) && !(un.absorbed_by >= 0 && ND[un.absorbed_by].blk.kind == B_DWS))) return false;
        const std::pair<int, int> f{n, un.cd.input_signed ? 1 : 0};
        if (std::find(fmts.begin(), fmts.end(), f) == fmts.end()) fmts.push_back(f);
    }
    return fmts.size() <= 2;
}

// pass 1
static void plan_residual_joins(f8_net* net) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    // ---- 1. residual fusion: an add rides in the epilogue of the LATER of its two producers when
    //         that producer is an MFMA conv nobody else reads and the other operand is already there.
    for (int i = 0; i < nn; ++i) {
        Node& ad = ND[i];
        if (ad.kind != N_ADD) continue;
        for (int pass = 0; pass < 2 && ad.fused_into < 0; ++pass) {
            const int x = pass == 0 ? ad.a : ad.b, y = pass == 0 ? ad.b : ad.a;
            const int px = T[x].prod, py = T[y].prod;
            Node& cx = ND[px];
            if (cx.kind != N_CONV || cx.cd.groups != 1 || cx.fused_add >= 0) continue;      // (any kernel, stride and pad)
            if (private_producer(net, x) < 0) continue;
            if (py > px) continue;     // other operand must exist before the conv runs
            ad.fused_into = px; cx.fused_add = i;
        }
    }
}

// pass 1b
static void plan_bottleneck_blocks(f8_net* net, int max_batch) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    const Options& opt = net->opt;
    const int fuse_blocks = opt.fuse_blocks;
    // ---- 1b. whole-block fusion: 1x1(ReLU) -> 3x3 pad 1 (ReLU) -> 1x1 + residual with the block input,
    //          all stride 1, intermediates read by nobody else  ->  one launch (f8_fused.hip)
    for (int i = 0; fuse_blocks && i < nn; ++i) {
        Node& c = ND[i];
        if (!plain_conv(c, 1, 1, 0) || c.fused_add < 0 || c.cd.relu || !c.cd.quant_input) continue;
        const int bi = private_producer(net, c.a);
        if (bi < 0) continue;
        Node& b = ND[bi];
        if (!plain_conv(b, 3, 1, 1) || b.fused_add >= 0 || !b.cd.quant_input) continue;
        const int ai = private_producer(net, b.a);
        if (ai < 0) continue;
        Node& a0 = ND[ai];
        // (a0.cd.quant_input is deliberately not asked for: without it body.0 reads the shift-0 int8 form of the block input (consumer_format), an int8
        //  form like any other to this launch; the chain launch asks for it, below)
        if (!plain_conv(a0, 1, 1, 0) || a0.fused_add >= 0) continue;
        if (join_other(net, c) != a0.a) continue;             // residual operand must be the block input
        const Tensor& x = T[a0.a];
        const int C = a0.cd.cin, MID = a0.cd.cout;
        if (c.cd.cout != C || b.cd.cin != MID || b.cd.cout != MID || c.cd.cin != MID) continue;
        int R = 0;
        const bool chainable = opt.fuse_chain && a0.cd.quant_input && chain_supported(C, MID, x.H, x.W, C) &&    // pass 1f decides; R = 0: no stand-alone launch
                               (opt.fuse_chain7 || !cchain_supported(C, MID, x.H, x.W, C, false));
        if (!fused_bottleneck_supported(C, MID, x.H, x.W, opt.whole_batch_launches ? max_batch : std::max(1, max_batch / opt.split), opt.fuse_stages, &R) && !chainable) {
            // no whole-block instance (the 7x7 maps of stage 3): body.0 + body.2 as one launch, the residual-carrying 1x1 stays
            if (opt.fuse_p12 && fused_p12_supported(C, MID, x.H, x.W) && a0.cd.relu && b.cd.relu) {
                set_block(net, bi, Block{B_P12, ai, bi});
                b.no_classes = true;
            }
            continue;
        }
        set_block(net, i, Block{B_BOTTLENECK, ai, bi, i, -1, false, R});
        b.no_classes = true;
    }
}

// pass 1c
static void plan_dual_gemm_joins(f8_net* net) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    const Options& opt = net->opt;
    // ---- 1c. downsample join: the add's two operands are both 1x1 / pad 0 convs (body.4 and the shortcut) and the
    //          earlier one feeds nothing else  ->  one dual-GEMM launch, its int32 result never touches HBM
    for (int i = 0; opt.fuse_dual && i < nn; ++i) {
        Node& h = ND[i];
        // (claimed(): after 1b a 1x1 conv that carries a join, h, can only host an identity bottleneck; one that carries none and feeds one add, g, only be absorbed)
        // (h and g at ANY stride, deliberately: the shortcut of a stride-2 opening block is a 1x1 / 2; the two output maps are compared below)
        if (!plain_conv(h, 1, h.cd.stride, 0) || h.fused_add < 0 || claimed(net, i)) continue;
        if (h.cd.cin % 64 != 0 || round_up(h.cd.cout, 32) <= 32) continue;          // kernel instances: BK = 64, BN = 64
        const int gi = private_producer(net, join_other(net, h));
        if (gi < 0) continue;
        Node& g = ND[gi];
        if (!plain_conv(g, 1, g.cd.stride, 0) || g.fused_add >= 0 || claimed(net, gi) || g.cd.relu || g.cd.cin % 64 != 0 || g.cd.cout != h.cd.cout) continue;
        if (T[g.out].H != T[h.out].H || T[g.out].W != T[h.out].W) continue;
        h.dual = gi; g.dual_host = i;
    }
}

// pass 1d
static void plan_stage_opening_blocks(f8_net* net) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    const Options& opt = net->opt;
    const int fuse_blocks = opt.fuse_blocks;
    // ---- 1d. stage-opening bottleneck at unchanged resolution: body.0 -> body.2 -> [body.4 + shortcut] in ONE launch
    for (int i = 0; fuse_blocks && i < nn; ++i) {
        Node& h = ND[i];
        if (h.kind != N_CONV || h.dual < 0 || (h.cd.stride != 1 && h.cd.stride != 2) || h.cd.relu || !h.cd.quant_input) continue;
        const int bs = h.cd.stride;                            // stride of the shortcut = stride of the block's 3x3
        Node& g = ND[h.dual];
        if (g.cd.stride != 1 || !g.cd.quant_input) continue;
        const int bi = private_producer(net, g.a);
        if (bi < 0) continue;
        Node& b = ND[bi];
        // (claimed: b feeds g, which carries no join — a P12 host (1b) feeds the conv that carries the block's; a0 is a 1x1 conv that carries no join: no host)
        if (!plain_conv(b, 3, bs, 1) || b.fused_add >= 0 || claimed(net, bi) || !b.cd.quant_input) continue;
        const int ai = private_producer(net, b.a);
        if (ai < 0) continue;
        Node& a0 = ND[ai];
        if (!plain_conv(a0, 1, 1, 0) || a0.fused_add >= 0 || claimed(net, ai) || !a0.cd.quant_input || a0.a != h.a || a0.dual >= 0) continue;
        const Tensor& x = T[h.a];
        int na = 0, nh = 0;
        if (consumer_format(x, a0.cd, &na, "finalize") || consumer_format(x, h.cd, &nh, "finalize")) continue;
        if (na != nh || a0.cd.input_signed != h.cd.input_signed) continue;      // one int8 form of the block input serves both
        const int C = a0.cd.cin, MID = a0.cd.cout;
        if (b.cd.cin != MID || b.cd.cout != MID || g.cd.cin != MID || g.cd.cout != h.cd.cout || h.cd.cin != C) continue;
        int R = 0;
        if (bs == 1 ? !(opt.fuse_ds && fused_ds_supported(C, MID, h.cd.cout, x.H, x.W, &R))
                    : !(opt.fuse_opener && fused_opener_supported(C, MID, h.cd.cout, x.H, x.W, &R))) continue;
        set_block(net, i, Block{B_OPENING, ai, bi, h.dual, i, bs == 2, R});
        b.no_classes = true;
    }
}

// pass 1f
static void plan_stage_chains(f8_net* net) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    const Options& opt = net->opt;
    const int fuse_blocks = opt.fuse_blocks;
    // ---- 1f. stage chains: consecutive bottleneck blocks at one resolution whose block-to-block tensors are read by nobody else
    //          -> ONE launch for all of them, the int32 residual stream stays in registers (f8_chain.hip).  A chain may start with
    //          the stage-opening block at unchanged resolution (1d) and continues through identity blocks (1b).
    if (opt.fuse_chain && fuse_blocks) {
        struct Blk { int host, in_t, out_t, C, MID, H, W, cin0; bool ds; bool tail = false; };
        auto block_of = [&](int i, Blk* bk) -> bool {
            const Node& h = ND[i];
            if (h.kind != N_CONV || h.fused_add < 0 || h.chain_into >= 0) return false;
            const Block& B = h.blk;                                // the blocks 1b and 1d marked are what a chain is made of
            if (B.kind == B_BOTTLENECK) {
                const Node& a0 = ND[B.b0]; const Tensor& x = T[a0.a];
                *bk = Blk{i, a0.a, ND[h.fused_add].out, a0.cd.cin, a0.cd.cout, x.H, x.W, a0.cd.cin, false};
                return true;
            }
            if (B.kind == B_OPENING && !B.s2) {
                const Node& a0 = ND[B.b0]; const Tensor& x = T[h.a];
                *bk = Blk{i, h.a, ND[h.fused_add].out, h.cd.cout, a0.cd.cout, x.H, x.W, a0.cd.cin, true};
                return true;
            }
            if (B.kind == B_OPENING && B.s2 && opt.fuse_tail) {
                // stage-opening block with a stride-2 3x3 (1d fused it on f8_opener.hip): candidate for body.0 + body.2 there and the JOIN as the
                // first block of the stage's chain (geometry of the chain = the block's OUTPUT map)
                // chain_kernel<TAIL> addresses the shortcut's operand as [N][2H][2W][CIN0]: only an input map of exactly twice the output's sides
                // (a 55x55 map also gives 28x28: the generic dual GEMM takes that one)
                const Node& a0 = ND[B.b0]; const Tensor& y = T[ND[h.fused_add].out]; const Tensor& x = T[h.a];
                if (x.H == 2 * y.H && x.W == 2 * y.W) {
                    *bk = Blk{i, h.a, ND[h.fused_add].out, h.cd.cout, a0.cd.cout, y.H, y.W, a0.cd.cin, true, true};
                    return true;
                }
            }
            if (h.dual >= 0 && B.kind != B_OPENING && plain_conv(h, 1, 2, 0) && h.cd.quant_input && opt.fuse_tail) {
                // the same for an opening block whose convs run as separate launches (stages 2 / 3 of ResNet-50; stage 1 when body.0 and the shortcut
                // read different int8 forms): the dual-GEMM join (1c) becomes the chain's first block, body.2's int8 output is its mid2
                const Node& g = ND[h.dual]; const Tensor& y = T[ND[h.fused_add].out]; const Tensor& x = T[h.a]; const Tensor& m2 = T[g.a];
                if (plain_conv(g, 1, 1, 0) && g.cd.quant_input && !g.cd.relu && !h.cd.relu &&      // (1c made the pair of plain 1x1 / pad 0 convs; the strides are asked here)
                    x.H == 2 * y.H && x.W == 2 * y.W && m2.H == y.H && m2.W == y.W) {
                    *bk = Blk{i, h.a, ND[h.fused_add].out, h.cd.cout, g.cd.cin, y.H, y.W, h.cd.cin, true, true};
                    return true;
                }
            }
            return false;
        };
        for (int i = 0; i < nn; ++i) {
            Blk first;
            if (!block_of(i, &first)) continue;
            if (first.tail ? !chain_tail_supported(first.C, first.MID, first.H, first.W, first.cin0) : !chain_supported(first.C, first.MID, first.H, first.W, first.cin0)) continue;
            if (!opt.fuse_chain7 && cchain_supported(first.C, first.MID, first.H, first.W, first.cin0, first.tail)) continue;
            std::vector<int> hosts{first.host};
            Blk cur = first;
            const int max_blocks = chain_max_blocks(first.C, first.MID, first.H, first.W, first.cin0, first.tail);
            while ((int)hosts.size() < max_blocks && !is_output(net, cur.out_t)) {
                const Tensor& y = T[cur.out_t];
                if (y.consumers.size() != 2) break;
                int next = -1;
                for (int j = cur.host + 1; j < nn && next < 0; ++j) {
                    Blk nb;
                    if (block_of(j, &nb) && !nb.ds && nb.in_t == cur.out_t) next = j;
                }
                if (next < 0) break;
                Blk nb; block_of(next, &nb);
                if (nb.C != first.C || nb.MID != first.MID || nb.H != first.H || nb.W != first.W) break;
                const int c0 = y.consumers[0], c1 = y.consumers[1], want0 = ND[next].blk.b0, want1 = ND[next].fused_add;
                if (!((c0 == want0 && c1 == want1) || (c0 == want1 && c1 == want0))) break;
                hosts.push_back(next); cur = nb;
            }
            if (hosts.size() < 2) continue;
            set_chain(net, hosts, C_STAGE);
            if (first.tail) {
                // the opener becomes: [body.0 + body.2 on f8_opener.hip (P12), host = the 3x3, output = mid2 in body.4's int8 format] + [the chain's first block]
                const Block o = ND[first.host].blk;
                if (o.kind == B_OPENING) {
                    release_block(net, first.host);
                    set_block(net, o.b2, Block{B_P12, o.b0, o.b2, -1, -1, true, o.R});
                    ND[o.b2].no_classes = true;
                }
                set_block(net, first.host, Block{B_JOIN, -1, -1, ND[first.host].dual, first.host});
            }
        }
        // identity blocks that only the chain kernel could run and that did not end up in a chain: back to separate launches
        for (int i = 0; i < nn; ++i) {
            const Node& c = ND[i];
            if (c.kind == N_CONV && c.blk.kind == B_BOTTLENECK && c.blk.R == 0 && c.chain_into < 0) release_block(net, i);
        }
    }
}

// pass 1g
static void plan_basic_block_chains(f8_net* net) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    const Options& opt = net->opt;
    const int fuse_blocks = opt.fuse_blocks;
    // ---- 1g. BasicBlock identity blocks (3x3 ReLU -> 3x3 + residual with the block input, all stride 1) -> f8_bchain.hip: ONE launch for
    //          the consecutive ones of a stage, the int32 stream in registers (a single block is a chain of one: both convs in one
    //          launch, `mid` only in LDS).  Option fuse_bchain7: the 7x7 x 512 stage the same way over clusters of eight workgroups (f8_bcchain.hip);
    //          value 2 puts the JOIN of the stage-opening block in front (its stride-2 body.0 stays a launch of its own)
    if ((opt.fuse_bchain || opt.fuse_bchain7) && fuse_blocks) {
        auto cluster7 = [&](int cc, const Tensor& t) { return opt.fuse_bchain7 && bcchain_supported(cc, t.H, t.W, false); };
        // (claimed(), here and below: the hosts so far carry a join — those of B_JOIN have `dual` —, or are a 3x3 that feeds a 1x1 conv (P12), which none of these does)
        auto bblock = [&](int i, int* in_t, int* out_t, int* C) -> bool {
            const Node& c2 = ND[i];
            if (!plain_conv(c2, 3, 1, 1) || c2.fused_add < 0 || claimed(net, i) || c2.dual >= 0 || c2.cd.relu || !c2.cd.quant_input) return false;
            const int c1i = private_producer(net, c2.a);
            if (c1i < 0) return false;
            const Node& c1 = ND[c1i];
            if (!plain_conv(c1, 3, 1, 1) || c1.fused_add >= 0 || claimed(net, c1i) || !c1.cd.quant_input || c1.dual >= 0) return false;
            if (join_other(net, c2) != c1.a) return false;
            const int cc = c1.cd.cin;
            if (c1.cd.cout != cc || c2.cd.cin != cc || c2.cd.cout != cc || cc % 32) return false;
            if (ND[T[c1.a].prod].kind == N_INPUT) return false;
            if (cluster7(cc, T[c1.a]) ? false : !(opt.fuse_bchain && bchain_supported(cc, T[c1.a].H, T[c1.a].W))) return false;
            *in_t = c1.a; *out_t = ND[c2.fused_add].out; *C = cc;
            return true;
        };
        for (int i = 0; i < nn; ++i) {
            int in_t, out_t, C;
            if (!bblock(i, &in_t, &out_t, &C)) continue;
            std::vector<int> hosts{i};
            const bool sgn0 = ND[T[ND[i].a].prod].cd.input_signed;
            int cur_out = out_t;
            while ((int)hosts.size() < kBChainMaxBlocks && !is_output(net, cur_out)) {
                const Tensor& y = T[cur_out];
                if (y.consumers.size() != 2) break;
                int next = -1, nin = -1, nout = -1, nC = 0;
                for (int j = hosts.back() + 1; j < nn && next < 0; ++j)
                    if (bblock(j, &nin, &nout, &nC) && nin == cur_out) next = j;
                if (next < 0 || nC != C) break;
                const int c1n = T[ND[next].a].prod;
                if (ND[c1n].cd.input_signed != sgn0) break;              // one border pattern for the int8 copy of the stream
                const int k0 = y.consumers[0], k1 = y.consumers[1], w0 = c1n, w1 = ND[next].fused_add;
                if (!((k0 == w0 && k1 == w1) || (k0 == w1 && k1 == w0))) break;
                hosts.push_back(next); cur_out = nout;
            }
            const bool cluster = cluster7(C, T[in_t]);
            for (int h : hosts) {
                Node& c2 = ND[h]; Node& c1 = ND[T[c2.a].prod];
                set_block(net, h, Block{B_BASIC, T[c2.a].prod, h});
                c1.no_classes = true; c2.no_classes = true;
            }
            // the stage-opening block in front of them (3x3 / 2 ReLU -> 3x3, 1x1 / 2 shortcut, join) joins the launch when the chain is
            // the only reader of its output (its two convs over the block input may read different int8 forms of it)
            [&] {
                if ((cluster ? opt.fuse_bchain7 : opt.fuse_bchain) < 2 || (int)hosts.size() >= kBChainMaxBlocks || is_output(net, in_t)) return;
                const Tensor& y = T[in_t];
                const int c1f = T[ND[i].a].prod, adf = ND[i].fused_add;
                if (y.consumers.size() != 2 || !((y.consumers[0] == c1f && y.consumers[1] == adf) || (y.consumers[0] == adf && y.consumers[1] == c1f))) return;
                if (ND[y.prod].kind != N_ADD || ND[y.prod].fused_into < 0) return;
                const int hi = ND[y.prod].fused_into;
                Node& h = ND[hi];
                if (!plain_conv(h, 1, 2, 0) || h.fused_add != y.prod || claimed(net, hi) || h.dual >= 0 || h.cd.relu || !h.cd.quant_input) return;
                const int gi = private_producer(net, join_other(net, h));
                if (gi < 0) return;
                Node& g = ND[gi];
                if (!plain_conv(g, 3, 1, 1) || g.fused_add >= 0 || claimed(net, gi) || g.dual >= 0 || g.cd.relu || !g.cd.quant_input) return;
                const int bi = private_producer(net, g.a);
                if (bi < 0) return;
                Node& b0 = ND[bi];
                if (!plain_conv(b0, 3, 2, 1) || b0.fused_add >= 0 || claimed(net, bi) || b0.dual >= 0 || !b0.cd.quant_input || b0.a != h.a) return;
                const Tensor& x = T[h.a];
                if (ND[x.prod].kind == N_INPUT || x.H != 2 * y.H || x.W != 2 * y.W) return;
                if (b0.cd.cin * 2 != C || h.cd.cin * 2 != C || b0.cd.cout != C || g.cd.cin != C || g.cd.cout != C || h.cd.cout != C) return;
                int na = 0, nh = 0;
                if (consumer_format(x, b0.cd, &na, "finalize") || consumer_format(x, h.cd, &nh, "finalize")) return;
                if (cluster) {                                           // only the join (body.2 + shortcut) joins the cluster launch; body.0 writes its 7x7 int8 output
                    if (!bcchain_supported(C, y.H, y.W, true)) return;
                    set_block(net, hi, Block{B_BASIC_JOIN, -1, gi, -1, hi});
                    g.no_classes = true;
                    hosts.insert(hosts.begin(), hi);
                    return;
                }
                if (!bchain_ds_supported(C, y.H, y.W)) return;
                set_block(net, hi, Block{B_BASIC_OPENING, bi, gi, -1, hi});
                b0.no_classes = true; g.no_classes = true;
                hosts.insert(hosts.begin(), hi);
            }();
            set_chain(net, hosts, cluster ? C_BASIC_CLUSTER : C_BASIC);
        }
    }
}

// The inverted residual that ends in project conv ci: 1x1 expand a0 -> depthwise b -> 1x1 project c [+ residual join with a0's input, res], every conv
// requantising its input, the two intermediates private; out = the block output.  Passes 1e, 1e3 and 1e2 share it and differ in
//   dw_ok    the depthwise geometry the pass's launch runs
//   rechain  what counts as taken.  false: whatever claimed() says, of all three convs.  true (1e2): c may host the B_IR block 1e made and the members may
//            be absorbed by c itself — 1e2 takes that block over —, and a0 may be the project conv of an inverted residual 1e2 CHAINED already (expand /
//            depthwise / project / expand ...: a conv is one block's project and no other's expand).  For the members 1e2 reads absorbed_by, not claimed():
//            a depthwise conv hosts nothing and has no dual, and a0's other marks are asked one by one.
struct IRBlock { int a0, b, c, out; bool res; };
static bool match_inverted_residual(const f8_net* net, int ci, bool (*dw_ok)(const Node&), bool rechain, IRBlock* k) {
    const auto& T = net->tensors; const auto& ND = net->nodes;
    const Node& c = ND[ci];
    // (claimed(): of the hosts before 1e only an identity bottleneck's is a stride-1 1x1 conv without `dual`, as c and a0 are; depthwise convs are the passes 1e .. 1k's alone)
    if (!plain_conv(c, 1, 1, 0) || !c.cd.quant_input || claimed(net, ci, rechain ? B_IR : B_NONE) || c.dual >= 0) return false;
    auto member_taken = [&](int m) { return rechain ? (ND[m].absorbed_by >= 0 && ND[m].absorbed_by != ci) : claimed(net, m); };
    const int bi = private_producer(net, c.a);
    if (bi < 0) return false;
    const Node& b = ND[bi];
    if (!dw_ok(b) || !b.cd.quant_input || b.fused_add >= 0 || member_taken(bi)) return false;
    const int ai = private_producer(net, b.a);
    if (ai < 0) return false;
    const Node& a0 = ND[ai];
    if (!plain_conv(a0, 1, 1, 0) || !a0.cd.quant_input || a0.fused_add >= 0 || member_taken(ai) || a0.dual >= 0) return false;
    if (rechain && (a0.dual_host >= 0 || (a0.blk.kind != B_NONE && !(a0.blk.kind == B_IR && a0.chain_into >= 0)))) return false;
    if (ND[T[a0.a].prod].kind == N_INPUT) return false;         // the network input has its own layouts
    *k = IRBlock{ai, bi, ci, c.out, false};
    if (c.fused_add >= 0) {                                       // a residual join must be with the block input, at stride 1
        if (join_other(net, c) != a0.a || b.cd.stride != 1) return false;
        k->res = true; k->out = ND[c.fused_add].out;
    }
    return true;
}

// pass 1e
static void plan_inverted_residuals(f8_net* net) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    const Options& opt = net->opt;
    // ---- 1e. MobileNet-V2 inverted residual: 1x1 expand (ReLU) -> depthwise 3x3 (ReLU) -> 1x1 project [+ residual with the
    //          block input], intermediates read by nobody else  ->  one launch (f8_ir.hip), the expanded tensors stay in LDS
    for (int i = 0; opt.fuse_ir && i < nn; ++i) {
        IRBlock k;
        if (!match_inverted_residual(net, i, [](const Node& b) { return depthwise_conv(b, 3, 1, true); }, false, &k)) continue;
        const Tensor& x = T[ND[k.a0].a];
        int R = 0, G = 0;
        if (!fused_ir_config(x.Cs, round_up(ND[i].cd.cout, 32), x.H, x.W, ND[k.b].cd.stride, &R, &G)) continue;
        if (opt.fuse_ir == 1) {
            // Where the fused launch wins (measured per block on MobileNet-V2 at 128 images, round 3 — after the depthwise phase moved to
            // the matrix cores and the requantisations to five operations; three launches / fused, us): stage 1 (112x112 / 2 and 56x56
            // maps: the 6x expanded tensor is 154 MB) 139.5 / 118.6 and 126.3 / 108.0; stage 2 (56x56 / 2, 28x28): 138 / 50.6, 69 / 40.4,
            // 68 / 38.7; stages 3 - 4 (28x28 / 2, 14x14): 44 / 30.5, 48 / 34.4, 46 / 33.3, 45 / 30.5, 51 / 37.4 and, with 576 expanded
            // channels, 49.1 / 46.3 and 46.1 / 43.3.  The 7x7 blocks (960 channels = 15 chunks over 49 pixels, 64 workgroups for 128
            // images) stay three launches: 34 - 40 / 90 - 114.  fuse_ir = 2 fuses every block that has an instance.
            if (T[ND[i].out].H * T[ND[i].out].W < 128) continue;
        }
        set_block(net, i, Block{B_IR, k.a0, k.b, i, -1, false, R, G});
    }
}

// pass 1e3
static void plan_inverted_residuals_k(f8_net* net) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    // ---- 1e3. (option fuse_irk) the inverted residual of MnasNet / ProxylessNAS / FBNet: 1x1 expand -> depthwise 5x5 or 7x7 / 1 or 2, pad K / 2 -> 1x1
    //           project [+ residual with the block input], intermediates read by nobody else and no output  ->  one launch (f8_irk.hip).  1e's conditions
    //           with the depthwise geometry exchanged; K = 3 / pad 1 stays 1e's (its choice to leave small maps unfused included), pad < K / 2 stays
    //           three launches.  Any format: the launch has a generic instance.
    for (int i = 0; net->opt.fuse_irk && i < nn; ++i) {
        IRBlock k;
        if (!match_inverted_residual(net, i, [](const Node& b) { return (b.cd.kernel == 5 || b.cd.kernel == 7) && depthwise_conv(b, b.cd.kernel, b.cd.kernel / 2, true); },
                                     false, &k)) continue;
        const Tensor& x = T[ND[k.a0].a];
        int R = 0, G = 0;
        if (!irk_config(ND[k.b].cd.kernel, x.Cs, round_up(ND[i].cd.cout, 32), x.H, x.W, ND[k.b].cd.stride, &R, &G)) continue;
        set_block(net, i, Block{B_IRK, k.a0, k.b, i, -1, false, R, G});
    }
}

// pass 1e2
static void plan_inverted_residual_chains(f8_net* net) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    const Options& opt = net->opt;
    // ---- 1e2. runs of >= 2 consecutive STRIDE-1 inverted residuals on one map  ->  ONE launch, one workgroup per image (f8_irchain.hip): the
    //           block outputs between them exist in no form at all (int8 block input and int32 stream in LDS).  It matches for itself: a block pass 1e
    //           left as three launches (the 7x7 maps under fuse_ir = 1) is taken as well, and the block 1e made of a chained one is released first.
    if (!opt.fuse_irchain) return;
    // the stride-1 block whose project conv is ci.  (Its map is the block input's: three stride-1 convs, 1x1 / pad 0 and 3x3 / pad 1.  A joined project
    // conv's result is read by the join alone: pass 1, the only writer of fused_add, asked for that.)
    auto match = [&](int ci, IRBlock* k) { return match_inverted_residual(net, ci, [](const Node& b) { return depthwise_conv(b, 3, 1, false); }, true, k); };
    // the widest block input / output and the widest int32 stream a block of the run joins: what irchain_supported checks
    auto fits = [&](const std::vector<IRBlock>& run) {
        const Tensor& x = T[ND[run[0].a0].a];
        int cin_max = 0, cout_max = 0, keep_max = 0;
        for (const IRBlock& k : run) {
            const int ci = T[ND[k.a0].a].Cs, co = round_up(ND[k.c].cd.cout, 32);
            cin_max = std::max(cin_max, ci); cout_max = std::max(cout_max, co);
            if (k.res) keep_max = std::max(keep_max, ci);
        }
        return (int)run.size() <= kIRChainMaxBlocks && irchain_supported(x.H, x.W, cin_max, cout_max, keep_max);
    };
    for (int i = 0; i < nn; ++i) {
        IRBlock k0;
        if (!match(i, &k0)) continue;
        std::vector<IRBlock> run{k0};
        if (!fits(run)) continue;
        for (;;) {                                                // extend: the block output's only readers are the next block's expand conv and its join
            const IRBlock& last = run.back();
            if (is_output(net, last.out)) break;
            const Tensor& o = T[last.out];
            int nxt = -1, joins = 0, others = 0;
            for (int u : o.consumers) {
                const Node& un = ND[u];
                if (un.kind == N_CONV && un.cd.groups == 1 && un.cd.kernel == 1) { if (nxt < 0) nxt = u; else ++others; }
                else if (un.kind == N_ADD) ++joins;
                else ++others;
            }
            if (nxt < 0 || others) break;
            // the next block: the project conv that consumes nxt's expand -> depthwise chain
            const Tensor& e1 = T[ND[nxt].out];
            if (e1.consumers.size() != 1) break;
            const Tensor& e2 = T[ND[e1.consumers[0]].out];
            if (e2.consumers.size() != 1) break;
            IRBlock kn;
            if (!match(e2.consumers[0], &kn) || kn.a0 != nxt || ND[kn.a0].a != last.out) break;
            if (joins != (kn.res ? 1 : 0)) break;
            if (kn.res && ND[ND[kn.c].fused_add].fused_into != kn.c) break;
            run.push_back(kn);
            if (!fits(run)) { run.pop_back(); break; }
        }
        if (run.size() < 2) continue;
        std::vector<int> hosts;
        for (const IRBlock& k : run) {
            if (ND[k.c].blk.kind != B_NONE) release_block(net, k.c);      // (pass 1e's block: its tile is the stand-alone launch's)
            set_block(net, k.c, Block{B_IR, k.a0, k.b, k.c});
            hosts.push_back(k.c);
        }
        set_chain(net, hosts, C_IR);
    }
}

// the 1x1 of a head launch (pass 1h) that only head_dws_kernel runs: more than one 32-channel output tile, or a ReLU
static bool head_dws_form(const Node& c) { return c.cd.relu || round_up(c.cd.cout, 32) != 32; }

// pass 1h
static void plan_mobilenet_v2_head(f8_net* net) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    const Options& opt = net->opt;
    // ---- 1h. MobileNet-V2 head: network input -> 3x3 / 2 conv (cin <= 4 -> 32, ReLU) -> depthwise 3x3 (ReLU) -> 1x1 (32 -> <= 32), each read
    //          by nobody else  ->  ONE row-walking launch (f8_stem.hip, stem_rows_kernel<KIND, true>): the three convs hand their rows to
    //          each other in registers, the launch reads the caller's buffer itself.  Option fuse_head_dws: the same position of MobileNet-V1 —
    //          the 1x1 may have up to 64 output channels and / or a ReLU (f8_head_dws.hip, head_dws_kernel<KIND, NT>; bind_step picks the kernel
    //          by those two properties); every other condition is the same.  Before 1j / 1k, which leave the claimed block 0 alone.
    for (int i = 0; (opt.fuse_head2 || opt.fuse_head_dws) && opt.fuse_stem && i < nn; ++i) {
        Node& c = ND[i];
        if (!plain_conv(c, 1, 1, 0) || !c.cd.quant_input || c.cd.input_signed || c.fused_add >= 0 || claimed(net, i) || c.dual >= 0 ||
            is_output(net, c.out)) continue;      // (claimed: a stride-1 1x1 conv that carries no join and has no `dual` hosts only B_IR)
        if (c.cd.cin != 32) continue;
        if (head_dws_form(c)) { if (!opt.fuse_head_dws || round_up(c.cd.cout, 32) > 64) continue; }      // MobileNet-V1's form
        else if (!opt.fuse_head2) continue;                                                                // MobileNet-V2's: no ReLU, <= 32 couts
        const int bi = private_producer(net, c.a);
        if (bi < 0) continue;
        const Tensor& tb = T[c.a];
        Node& b = ND[bi];
        // (b and h: absorbed_by is all of claimed() here — a depthwise conv hosts nothing and has no dual, and the one 3x3 / 2 host, a stride-2 P12's, reads
        //  a 1x1 conv's output, not the network input.  32 channels: more than one, as depthwise_conv asks, and as many outputs, as add_conv_node does)
        if (!depthwise_conv(b, 3, 1, false) || b.cd.cin != 32 || !b.cd.relu || !b.cd.quant_input || b.cd.input_signed || b.fused_add >= 0 || b.absorbed_by >= 0) continue;
        const int hi = private_producer(net, b.a);
        if (hi < 0) continue;
        const Tensor& ta = T[b.a];
        Node& h = ND[hi];
        if (!plain_conv(h, 3, 2, 1) || h.cd.cin > 4 || h.cd.cout != 32 || !h.cd.relu || h.fused_add >= 0 || h.absorbed_by >= 0 || is_output(net, h.a)) continue;
        const Tensor& x = T[h.a];
        if (ND[x.prod].kind != N_INPUT || x.consumers.size() != 1 || !(!h.cd.quant_input || x.fl == h.cd.input_fl)) continue;
        if (!head2_supported(x.H, x.W) || ta.H * 2 != x.H || ta.W * 2 != x.W) continue;
        int na = 0, nb2 = 0;
        if (consumer_format(ta, b.cd, &na, "finalize") || consumer_format(tb, c.cd, &nb2, "finalize") || na < 1 || nb2 < 1 || na > 16 || nb2 > 16) continue;
        // 16: kRequantU8MaxShift (the launch's float-converter form; accumulators the planner cannot bound take its integer form: rq_int)
        bool int8_readers = !T[c.out].consumers.empty() && T[c.out].consumers.size() <= 2;
        for (int u : T[c.out].consumers) if (ND[u].kind != N_CONV || !ND[u].cd.quant_input) int8_readers = false;
        if (!int8_readers) continue;
        set_block(net, i, Block{B_HEAD2, hi, bi, i});
    }
}

// pass 1i
static void plan_last_conv_and_pool(f8_net* net) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    const Options& opt = net->opt;
    // ---- 1i. the network's last 1x1 conv (hosting its residual join, or a plain conv + ReLU) and the average pool behind it: ONE launch that sums the map's
    //          pixels in the epilogue (f8_pool.hip); the conv's int32 result — read by nobody but the pool — never exists
    for (int i = 0; opt.fuse_pool && i < nn; ++i) {
        Node& p = ND[i];
        if (p.kind != N_AVGPOOL) continue;
        int ci = private_producer(net, p.a);
        if (ci < 0) continue;
        const Tensor& t = T[p.a];
        if (ND[ci].kind == N_ADD) { if (ND[ci].fused_into < 0) continue; ci = ND[ci].fused_into; }
        Node& c = ND[ci];
        if (c.kind == N_CONV && c.chain_into == ci && c.chain_kind == C_BASIC_CLUSTER && c.fused_add >= 0 && ND[c.fused_add].out == p.a && !is_output(net, p.out)) {
            c.pool = i; p.pool_host = ci;                         // the last block of a 7x7 BasicBlock cluster chain: the same (f8_bcchain.hip)
            continue;
        }
        if (c.kind == N_CONV && c.chain_into == ci && c.chain_kind == C_STAGE && c.fused_add >= 0 && ND[c.fused_add].out == p.a && !is_output(net, p.out) &&
            cchain_supported(c.cd.cout, c.cd.cin, t.H, t.W, c.cd.cout, false)) {      // (geometry: a chain's last block is an identity block)
            c.pool = i; p.pool_host = ci;                         // the last block of a 7x7 cluster chain: the pool is summed from its stream registers (f8_cchain.hip)
            continue;
        }
        if (!plain_conv(c, 1, 1, 0) || claimed(net, ci) || c.dual >= 0 || !c.cd.quant_input) continue;
        if ((c.fused_add >= 0 ? ND[c.fused_add].out : c.out) != p.a) continue;
        if (c.fused_add < 0 && T[c.out].consumers.size() != 1) continue;
        const int ckp = round_up(c.cd.cin, 32), coutP = round_up(c.cd.cout, 32);
        if (!conv1x1_pool_supported(ckp, coutP, t.H * t.W)) continue;
        c.pool = i; p.pool_host = ci;
    }
}

// The depthwise-separable block that ends in 1x1 conv ci (passes 1j and 1k): depthwise 3x3 / 1 or 2, pad 1, ReLU -> 1x1 [ReLU], both requantising their
// input, neither taken or linked to anything else, the depthwise result private, the block input not the network's, the block output no network output
// and read by somebody.  Returns the depthwise conv, -1: no such block.
static int match_depthwise_separable(const f8_net* net, int ci) {
    const auto& T = net->tensors; const auto& ND = net->nodes;
    const Node& c = ND[ci];
    if (!plain_conv(c, 1, 1, 0) || !c.cd.quant_input || c.fused_add >= 0 || c.dual >= 0 || c.pool >= 0 || claimed(net, ci)) return -1;
    const int bi = private_producer(net, c.a);
    if (bi < 0) return -1;
    const Node& b = ND[bi];
    if (!depthwise_conv(b, 3, 1, true) || !b.cd.relu || !b.cd.quant_input || b.fused_add >= 0 || claimed(net, bi)) return -1;
    const Tensor& x = T[b.a];
    if (ND[x.prod].kind == N_INPUT) return -1;                                        // the network input has its own layouts
    // whole 32-channel slices of REAL channels: a 48-channel block input has a 64-channel form, which dws_supported / dws7_supported — asked with Cs — would take
    if (b.cd.cin & 31) return -1;
    if (is_output(net, c.out) || T[c.out].consumers.empty()) return -1;              // the net output is int32
    if (T[c.a].H * b.cd.stride != x.H || T[c.a].W * b.cd.stride != x.W) return -1;   // (stride 2: an even map)
    return bi;
}

// pass 1j
static void plan_depthwise_separable(f8_net* net, int max_batch) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    // ---- 1j. MobileNet-V1 depthwise-separable block (option fuse_dws): depthwise 3x3 / 1 or 2, pad 1 (ReLU) -> 1x1 [ReLU], the depthwise result read
    //          by nobody else  ->  ONE launch (f8_dws.hip), the depthwise result only ever in LDS.  Behind every pass but 1k: whatever an earlier one
    //          claimed (MobileNet-V2's head and inverted residuals, the 1x1 + average pool) stays what it is.  The launch writes int8 forms only, so
    //          every reader of the block output must be a conv of its own (or another block of this kind) that requantises its input, in at most two formats.
    for (int i = 0; net->opt.fuse_dws && i < nn; ++i) {
        const int bi = match_depthwise_separable(net, i);
        if (bi < 0 || !int8_readers_only(net, ND[i].out)) continue;
        const Tensor& x = T[ND[bi].a];
        int R = 0;
        if (!dws_supported(x.Cs, round_up(ND[i].cd.cout, 32), x.H, x.W, ND[bi].cd.stride, max_batch, &R)) continue;      // (7-wide maps: no matrix-core walker form; pass 1k)
        set_block(net, i, Block{B_DWS, bi, -1, i, -1, false, R});
    }
}

// pass 1k
static void plan_depthwise_separable_7x7(f8_net* net, int max_batch) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    // ---- 1k. the same block on a 7 x 7 OUTPUT map (option fuse_dws7; f8_dws7.hip), which 1j's launch has no form for: 1j's conditions, and in addition
    //          a block output whose only reader is the average pool, itself not the net output — the pool is then summed in the launch (pool / pool_host, as 1i)
    //          and the block output exists in no form.  After 1j, so the last of the passes 1x: whatever an earlier one claimed stays claimed.
    for (int i = 0; net->opt.fuse_dws7 && i < nn; ++i) {
        const int bi = match_depthwise_separable(net, i);
        if (bi < 0) continue;
        Node& c = ND[i];
        const Tensor& x = T[ND[bi].a];
        // an inverted residual — expanding 1x1 (ReLU) -> depthwise -> 1x1 WITHOUT ReLU — is passes 1e / 1e2's to decide: the 7x7 ones that fuse_ir = 1
        // leaves as three launches were measured there (1j never sees them: it has no 7-wide form)
        const Node& xp = ND[x.prod];
        if (!c.cd.relu && xp.kind == N_CONV && xp.cd.groups == 1 && xp.cd.kernel == 1 && xp.cd.relu && xp.cd.cout > xp.cd.cin && x.consumers.size() == 1) continue;
        int pool = -1;
        if (T[c.out].consumers.size() == 1 && ND[T[c.out].consumers[0]].kind == N_AVGPOOL) {
            const int pi = T[c.out].consumers[0];
            if (ND[pi].pool_host >= 0 || is_output(net, ND[pi].out)) continue;             // (a pooled net output is int32 of the caller's: the pool stays a launch, and so does this conv's int32 result)
            pool = pi;
        }
        if (pool < 0 && !int8_readers_only(net, c.out)) continue;
        int I = 0;
        if (!dws7_supported(x.Cs, round_up(c.cd.cout, 32), x.H, x.W, ND[bi].cd.stride, max_batch, pool >= 0, &I)) continue;
        set_block(net, i, Block{B_DWS, bi, -1, i, -1, false, 0, 0, I});
        if (pool >= 0) { c.pool = pool; ND[pool].pool_host = i; }
    }
}

// pass 2
// The mode rule of the gathers — concat, nearest upsample, slice / shuffle, depth_to_space / space_to_depth.  Bytes mode: the result exists in one or two int8 forms
// and nothing else (no int32 reader, no network output: int8_forms_only); the sources are then asked for the result's formats and the launch moves
// bytes.  Otherwise the sources are read as int32 (ask_sources).  Replication and channel selection commute with every element-wise function, the
// requantisation among them, so upsample and a stand-alone slice / shuffle need no more; a concat also aligns fraclens and needs requant_commutes.
static bool int8_forms_only(const f8_net* net, int t) {
    const Tensor& o = net->tensors[t];
    int n8 = 0;
    for (auto& F : o.forms) n8 += F.kind == FORM_I8;
    return n8 >= 1 && n8 <= 2 && (int)o.forms.size() == n8 && !is_output(net, t);
}
// Conditions (c) - (e) of 4.5i: requantising operand i directly by n_i = n - (fl_ref - fl_i) is the same function as aligning it to fl_ref and
// requantising by n, for every n of `forms`.  The aligned value neither wraps nor clamps (stream_bounded on tensor t, the concat's result), for n > 0
// the reference's `v + 2^(n-1)` stays below 2^31 on it, and every n_i is a shift the kernels have (-31 .. 30).
static bool requant_commutes(f8_net* net, const std::vector<int>& srcs, int t, const std::vector<Form>& forms) {
    const int64_t amax = tensor_amax(net, t);
    if (!stream_bounded(net, t)) return false;
    for (const Form& F : forms) {
        if (F.n > 0 && amax + (int64_t(1) << (F.n - 1)) > INT32_MAX) return false;
        for (int x : srcs) { const int ni = F.n - (net->tensors[t].fl - net->tensors[x].fl); if (ni < -31 || ni > 30) return false; }
    }
    return true;
}
// asks every source for its int32 form or, in bytes mode, for `forms` (the result's) shifted by fl_ref - fl_i (0 for upsample and a stand-alone slice / shuffle)
static void ask_sources(f8_net* net, const std::vector<int>& srcs, int fl_ref, const std::vector<Form>& forms, bool bytes_mode) {
    for (int x : srcs) {
        Tensor& s = net->tensors[x];
        if (!bytes_mode) { add_form(s, FORM_I32, 0, 0); continue; }
        for (const Form& F : forms) add_form(s, FORM_I8, F.n - (fl_ref - s.fl), F.sgn);
    }
}

// Option fuse_table.  1: the measured rule (profiles/table_r15.md, batch 128, EfficientNet-B0's shapes): the fused launch is 1.07 - 1.59 x faster than
// the two launches on every shape up to 144 x 56 x 56 = 451 584 values an image and slower (0.96 x) on the one above, 96 x 112 x 112 = 1 204 224 —
// so it fuses below 2^20 values an image.  2: always (what the measurement ran).  0: never.
static bool fuse_table_rule(int opt, const Tensor& a) { return opt == 2 || (opt == 1 && (int64_t)a.C * a.H * a.W < (int64_t(1) << 20)); }

static void plan_tensor_forms(f8_net* net, int max_batch) {
    auto& T = net->tensors;
    auto& ND = net->nodes;
    const int nn = (int)ND.size();
    const Options& opt = net->opt;
    // ---- 2. which forms does each tensor need?  (reverse order: consumers before producers)
    if (!net->outs[0].idx) {
        const int out0 = net->outs[0].t;
        Tensor& O = T[out0];
        const Node& p = ND[O.prod];
        // the classifier (a linear / 1x1 conv on a 1x1 map that nothing else reads) writes the caller's buffer itself: no int32 form
        // (an argmax output on the same tensor reads the int32 form: the classifier then writes that, and the output launch copies it out)
        const Tensor& ps = T[p.a >= 0 ? p.a : out0];
        O.dense_out = opt.fuse_fc && (p.kind == N_LINEAR || p.kind == N_CONV) && p.cd.kernel == 1 && p.cd.stride == 1 && p.cd.pad == 0 && p.cd.groups == 1 &&
                      O.H == 1 && O.W == 1 && ps.H == 1 && ps.W == 1 && O.consumers.empty() && p.fused_add < 0 && p.absorbed_by < 0 && !p.cd.relu &&
                      fc_dense_supported(ps.Cs, round_up(p.cd.cout, 32)) && argmax_index(net, out0) < 0;
        if (!O.dense_out) add_form(O, FORM_I32, 0, 0);
    }
    for (size_t k = 0; k < net->outs.size(); ++k) {
        const int t = net->outs[k].t;
        if (!net->outs[k].idx) { if (k >= 1) add_form(T[t], FORM_I32, 0, 0); continue; }      // the copy-out launch reads the int32 form
        // An argmax output.  On an upsample's result that NOTHING else reads — no consumer, no value output — the argmax launch interpolates per output
        // pixel itself (option fuse_argmax): the upsample emits no launch, its result gets no form, its source is read in int32.  Its items
        // are indexed in 32 bits: the launch stays below 2^31 output pixels.  Otherwise the launch reads the marked tensor's int32 form, as a tap does.
        Node& p = ND[T[t].prod];
        if (opt.fuse_argmax && p.kind == N_UPSAMPLE && T[t].consumers.empty() && output_index(net, t) < 0 && (int64_t)max_batch * T[t].H * T[t].W < (int64_t(1) << 31)) {
            p.argmax_k = (int)k;
            add_form(T[p.a], FORM_I32, 0, 0);
        } else {
            add_form(T[t], FORM_I32, 0, 0);
        }
    }
    for (int i = nn - 1; i >= 0; --i) {
        Node& nd = ND[i];
        switch (nd.kind) {
            case N_CONV: case N_LINEAR: {
                Tensor& s = T[nd.a];
                int n = 0;
                consumer_format(s, nd.cd, &n, "finalize");
                nd.depthwise = nd.cd.groups != 1 && nd.cd.groups == nd.cd.cin;
                nd.grouped = nd.cd.groups != 1 && !nd.depthwise;      // (no matcher claims it: a launch of its own, its int8 input and its outputs in HBM)
                // nd inside a fused block: does its source exist in HBM at all, and which form of the stream does the launch read?
                int host = -1;
                const Role role = role_in_block(net, i, &host);
                const BlockKind bk = role != R_NONE ? ND[host].blk.kind : B_NONE;
                const int pos = chain_pos(net, host);            // of its block in a chain launch: the tensors between a chain's blocks exist in no form at all
                auto stream = [&]() -> Tensor& { return T[join_other(net, nd)]; };   // the other operand of nd's join
                bool in_launch = true;                           // nd's source lives in LDS / registers inside the launch: no HBM form
                switch (bk) {
                    case B_OPENING: in_launch = role == R_B2 || role == R_B4; break;      // (body.0 and the shortcut read the block input)
                    case B_P12: in_launch = role == R_B2; break;
                    case B_HEAD2: in_launch = role != R_B0; break;
                    case B_DWS: in_launch = role == R_B4; break;      // (the depthwise conv reads the block input from HBM)
                    case B_BASIC_JOIN:                           // (cluster launch: body.0's int8 output in HBM)
                        if (role == R_B2) add_form(s, FORM_I8, n, nd.cd.input_signed ? 1 : 0);
                        [[fallthrough]];
                    case B_BASIC_OPENING: in_launch = role == R_B2; break;      // (its 3x3 / 2 and its shortcut conv each ask for their int8 form of the block input below)
                    case B_BASIC:                                // the first conv's int8 input is made in the launch from the stage's int32 stream: the chain's only input form
                        if (role == R_B2 && pos == 0) add_form(stream(), FORM_I32, 0, 0);
                        break;
                    case B_IR:                                   // in a chain (f8_irchain.hip) only the first block's input exists in HBM: int8, and int32 when it joins it
                        in_launch = pos >= 0 || role != R_B0;    // (alone: the expand conv reads the block input from HBM)
                        if (pos == 0 && role == R_B0) add_form(s, FORM_I8, n, nd.cd.input_signed ? 1 : 0);
                        if (pos <= 0 && role == R_B4 && nd.fused_add >= 0) add_form(stream(), FORM_I32, 0, 0);
                        break;
                    case B_IRK:                                  // the expand conv reads the block input from HBM; a join reads its int32 form
                        in_launch = role != R_B0;
                        if (role == R_B4 && nd.fused_add >= 0) add_form(stream(), FORM_I32, 0, 0);
                        break;
                    case B_BOTTLENECK:                           // in a chain (f8_chain.hip) an identity first block reads only the int32 form of the stage input
                        if (role == R_B0) { in_launch = pos >= 0; if (pos == 0) add_form(s, FORM_I32, 0, 0); }      // (alone: it reads the block input from HBM)
                        if (role == R_B4 && pos <= 0) add_form(stream(), FORM_I32, 0, 0);
                        break;
                    default: in_launch = false;                  // a conv of its own; B_JOIN: the shortcut and body.4 read their int8 inputs from HBM
                }
                if (in_launch) break;
                nd.stem = !nd.depthwise && !nd.grouped && nd.cd.cin <= 4 && ND[s.prod].kind == N_INPUT && nd.cd.kernel <= 8 && nd.dil == 1 && !nd.rect &&
                          s.consumers.size() == 1 && !is_output(net, nd.a) && n == 0;
                if (nd.stem) {
                    const int Q = T[nd.out].W;
                    const int f = add_form(s, FORM_STEM, 0, 0);
                    Form& F = s.forms[f];
                    F.sgn = nd.cd.input_signed ? 1 : 0;
                    const bool h2 = bk == B_HEAD2;
                    F.pad = nd.cd.pad + (nd.sp_pool >= 0 ? 2 : 0) + (h2 ? 4 : 0);      // fused stem + pool: 2 more halo pixels keep every tile's patch in memory (head launch of MobileNet-V2: 5 in all)
                    F.Hp = s.H + 2 * F.pad;
                    F.Wp = round_up(std::max(s.W + 2 * F.pad, nd.cd.stride * (Q - 1) + 8), (nd.sp_pool >= 0 || h2) ? 4 : 2);
                } else {
                    add_form(s, FORM_I8, n, nd.cd.input_signed ? 1 : 0);
                }
                if (nd.fused_add >= 0 && nd.dual < 0 && bk != B_BASIC_OPENING && bk != B_BASIC_JOIN) add_form(stream(), FORM_I32, 0, 0);
                break;
            }
            case N_DECONV: {
                // reads its source as a conv of its own does: the int8 form in its consumer format, written by the source's producer in its epilogue
                // (a third format of one tensor: a requant: step from the int32 form, select_outputs).  No matcher counts it among a block's readers, so
                // a source inside a would-be fused launch is no private intermediate and the launch is cut there, as by an output tap.
                int n = 0;
                consumer_format(T[nd.a], nd.cd, &n, "finalize");
                add_form(T[nd.a], FORM_I8, n, nd.cd.input_signed ? 1 : 0);
                break;
            }
            case N_ADD:
                if (nd.fused_into < 0) { add_form(T[nd.a], FORM_I32, 0, 0); add_form(T[nd.b], FORM_I32, 0, 0); }
                break;
            case N_MAXPOOL: {
                Tensor& o = T[nd.out];
                if (!o.forms.empty() && T[nd.a].consumers.size() == 1 && !is_output(net, nd.a)) {
                    // ResNet head: 7x7/2 stem conv + this pool in one launch (the conv output never leaves LDS)
                    Node& c = ND[T[nd.a].prod];
                    if (c.kind == N_CONV && c.cd.groups == 1 && c.dil == 1 && !c.rect && c.fused_add < 0 && ND[T[c.a].prod].kind == N_INPUT && T[c.a].consumers.size() == 1 &&
                        !is_output(net, c.a) && (!c.cd.quant_input || T[c.a].fl == c.cd.input_fl) && opt.fuse_stem &&
                        stem_pool_supported(c.cd.cin, c.cd.cout, c.cd.kernel, c.cd.stride, c.cd.pad, nd.pk, nd.pstride, nd.ppad, o.H, o.W, opt.stem_rows, T[c.a].H, T[c.a].W)) {
                        c.sp_pool = i; nd.sp_conv = T[nd.a].prod;
                        break;                                   // no HBM form of the conv output
                    }
                }
                if (o.forms.size() == 1 && o.forms[0].kind == FORM_I8)
                    add_form(T[nd.a], FORM_I8, o.forms[0].n, o.forms[0].sgn);
                else
                    add_form(T[nd.a], FORM_I32, 0, 0);
                break;
            }
            case N_AVGPOOL:
                if (nd.pool_host < 0) add_form(T[nd.a], FORM_I32, 0, 0);      // fused behind its conv (1i): the pool's input has no form
                break;
            case N_CONCAT: {
                if (nd.cat_into >= 0) break;                     // the shuffle behind it reads the operands itself and asked them for its forms (N_SHUFFLE below, a later node)
                // the mode rule with conditions (c) - (e); they are evaluated first, whatever the mode: that bounds the stream (tensor_amax caches) here
                const Tensor& o = T[nd.out];
                const bool exact = requant_commutes(net, nd.srcs, nd.out, o.forms);
                nd.bytes_mode = opt.concat_i8 && int8_forms_only(net, nd.out) && exact;
                ask_sources(net, nd.srcs, o.fl, o.forms, nd.bytes_mode);
                break;
            }
            case N_SUMPOOL:
                // reads the source's int32 form, whatever reads the result.  No matcher counts it among a block's readers, so a source
                // inside a would-be fused launch is no private intermediate and the launch is cut there, as by an output tap.  The kernel: option sumpool_wide.
                add_form(T[nd.a], FORM_I32, 0, 0);
                nd.sum_wide = opt.sumpool_wide == 2 ? nd.sum_k >= 2 : opt.sumpool_wide == 1 && sumpool_wide_rule(nd.sum_k, nd.sum_stride);
                break;
            case N_SLICE: case N_SHUFFLE: {
                // the mode rule alone: the fraclen is the source's and no bound on the values is needed
                const Tensor& o = T[nd.out];
                nd.bytes_mode = opt.chanmap_i8 && int8_forms_only(net, nd.out);
                // concat -> shuffle in one launch (option fuse_shuffle): the concat is read by this shuffle alone, has `groups` operands of one width —
                // group i of the shuffle is then operand i — and its own conditions (c) - (e) hold for each of the shuffle's forms.  The operands are
                // asked for the forms a concat in bytes mode asks for; the concat gets no form and no launch.
                const Tensor& s = T[nd.a];
                Node& cat = ND[s.prod];
                bool fuse = nd.kind == N_SHUFFLE && nd.bytes_mode && opt.fuse_shuffle && cat.kind == N_CONCAT && s.consumers.size() == 1 && !is_output(net, nd.a) &&
                            (int)cat.srcs.size() == nd.cm_groups && requant_commutes(net, cat.srcs, nd.a, o.forms);
                for (size_t k = 0; fuse && k < cat.srcs.size(); ++k) fuse = T[cat.srcs[k]].C == o.C / nd.cm_groups;
                if (fuse) { nd.cm_cat = s.prod; cat.cat_into = i; }
                ask_sources(net, nd.cm_cat >= 0 ? cat.srcs : std::vector<int>{nd.a}, s.fl, o.forms, nd.bytes_mode);
                break;
            }
            case N_D2S: case N_S2D:
                // the mode rule alone, as a stand-alone slice / shuffle: a permutation of the source's values at the source's fraclen
                nd.bytes_mode = opt.pixmap_i8 && int8_forms_only(net, nd.out);
                ask_sources(net, {nd.a}, T[nd.a].fl, T[nd.out].forms, nd.bytes_mode);
                break;
            case N_MUL: {
                // reads like a conv with quant_input = 1: each operand's int8 form in the mul's format for it, written by the operand's producer (a == b in two
                // formats: two forms of one tensor; a third format on a tensor: a requant: step, select_outputs).  A hard gate that only this mul's b operand
                // reads (option fuse_hgate) runs inside the launch, which then reads the GATE's source in int32; the gate gets no form and no launch.
                Tensor& A = T[nd.a]; Tensor& B = T[nd.b];
                add_form(A, FORM_I8, A.fl - nd.md.a_fl, nd.md.a_signed);
                Node& gp = ND[B.prod];
                if (opt.fuse_hgate && gp.kind == N_HGATE && B.consumers.size() == 1 && nd.a != nd.b && !is_output(net, nd.b)) {
                    nd.mul_gate = B.prod; gp.gate_into = i;
                    add_form(T[gp.a], FORM_I32, 0, 0);
                } else if (fuse_table_rule(opt.fuse_table, A) && gp.kind == N_TABLE && B.consumers.size() == 1 && !is_output(net, nd.b) && B.H * B.W == 1 && A.H * A.W > 1) {
                    // a table that only this BROADCAST mul's b operand reads (the sigmoid SE gate): the launch reads the table's source bytes and looks
                    // them up in a byte table composed for (b_fl, b_signed); the table gets no form and no launch
                    nd.mul_table = B.prod; gp.tab_into = i;
                    add_form(T[gp.a], FORM_I8, T[gp.a].fl - gp.td.in_fl, gp.td.in_signed);
                } else {
                    add_form(B, FORM_I8, B.fl - nd.md.b_fl, nd.md.b_signed);
                }
                break;
            }
            case N_HGATE:
                if (nd.gate_into < 0) add_form(T[nd.a], FORM_I32, 0, 0);      // (fused: the mul, a later node, asked the source already)
                break;
            case N_TABLE:
                // reads like a conv with quant_input = 1: the source's int8 form in the index format, written by the source's producer.  The mode rule of
                // the gathers: bytes where the result exists in one or two int8 forms and nothing else.  No bound on values is needed: the entries are known.
                if (nd.tab_into >= 0) break;                                  // (fused: the mul, a later node, asked the source already)
                add_form(T[nd.a], FORM_I8, T[nd.a].fl - nd.td.in_fl, nd.td.in_signed);
                nd.bytes_mode = opt.table_i8 && int8_forms_only(net, nd.out);
                break;
            case N_UPSAMPLE: {
                if (nd.argmax_k >= 0) break;                                  // (fused: the argmax output asked the source for its int32 form above)
                // the mode rule alone, for nearest: the fraclen — so the shift — is the source's and no bound on the values is needed
                nd.bytes_mode = opt.upsample_i8 && nd.up_mode == F8_UP_NEAREST && int8_forms_only(net, nd.out);
                ask_sources(net, {nd.a}, T[nd.a].fl, T[nd.out].forms, nd.bytes_mode);
                break;
            }
            default: break;
        }
    }
}

// pass 3: the launches in node order, one emitter per launch family.  Each fills one Step: its input / output forms, the packed weights, the
// algorithmic bytes / ops / essential vector work, the name.  The weight image assigns offsets in call order: every emitter packs its convs in
// role order (Block), the order the plans were made with.

// conv c's input: the tensor (*t) and its form in c's int8 consumer format (*f; pass 2 made it)
static int conv_input_i8(const f8_net* net, const Node& c, int* t, int* f) {
    int n = 0;
    if (const int rc = consumer_format(net->tensors[c.a], c.cd, &n, "finalize")) return rc;
    *t = c.a; *f = find_form(net->tensors[c.a], FORM_I8, n, c.cd.input_signed ? 1 : 0);
    return F8_OK;
}
// a residual join (a << acc_shl) + (b << res_shl): dfl = fraclen of a - fraclen of b, the operand with the smaller fraclen shifts left
static void join_shifts(int dfl, int32_t* acc_shl, int32_t* res_shl) { *acc_shl = dfl < 0 ? -dfl : 0; *res_shl = dfl > 0 ? dfl : 0; }
// the tensor a conv's launch writes: the output of the residual join it hosts (the step applies its ReLU), else its own
static int join_output(const f8_net* net, const Node& c, Step& st) {
    if (c.fused_add < 0) return c.out;
    st.relu1 = net->nodes[c.fused_add].relu;
    return net->nodes[c.fused_add].out;
}
// bytes of a conv's packed weights + bias (depthwise: K * K taps + 4 bytes of bias per channel; grouped: the weights of the groups, not the zeros between them)
static double weight_bytes(const f8_net* net, const Node& c) {
    const f8_conv_geom g = geom_of(c);
    if (c.grouped) return (double)c.cd.cout * ((c.cd.cin / c.cd.groups) * g.kh * g.kw + 4);
    return c.depthwise ? (double)net->tensors[c.a].Cs * (g.kh * g.kw + 4) : (double)c.coutP * (c.ktot + 4);
}
// multiply-adds x 2 of a conv per image
static double conv_ops(const f8_net* net, const Node& c) {
    const Tensor& o = net->tensors[c.out];
    const f8_conv_geom g = geom_of(c);           // (a rectangular conv: its kh x kw real taps)
    return 2.0 * o.H * o.W * c.cd.cout * (c.cd.cin / c.cd.groups) * g.kh * g.kw;
}
// bytes per image a step writes: its output forms over px pixels of map o
static double out_bytes(const Step& st, const Tensor& o, double px) { return px * o.Cs * ((st.out.f32 >= 0 ? 4 : 0) + out_forms8(st)); }
// packs a block's convs in role order (frag: also in MFMA-fragment order) and adds their ops / weight bytes to the step
static void pack_block(f8_net* net, const Block& r, bool frag, Step& st) {
    for (int c : {r.b0, r.b2, r.b4, r.sc}) {
        if (c < 0) continue;
        Node& n = net->nodes[c];
        if (!n.depthwise) pack_conv_weights(net, n);
        else if (dw_general(n)) pack_dwk_weights(net, n);      // (the 5x5 / 7x7 of a B_IRK block)
        else pack_dw_weights(net, n);
        if (frag) pack_frag_weights(net, n);
        st.ops_per_img += conv_ops(net, n); st.bytes_const += weight_bytes(net, n);
    }
}
// "body.0+body.2+..." of a block's output tensors, role order
static std::string block_names(const f8_net* net, const Block& r) {
    std::string s;
    for (int c : {r.b0, r.b2, r.b4, r.sc}) if (c >= 0) s += (s.empty() ? "" : "+") + tname(net, net->nodes[c].out);
    return s;
}

// The tensor whose forms the launch hosted by conv c writes, t — or, where the plan folded the average pool behind it into the launch (c.pool; 1i, 1k), the
// POOLED tensor: the launch sums the map's pixels, so the step's outputs are that tensor's forms (its int32 form if nobody asked for another)
static int pooled_output(f8_net* net, const Node& c, int t) {
    if (c.pool < 0) return t;
    const int pt = net->nodes[c.pool].out;
    if (net->tensors[pt].forms.empty()) add_form(net->tensors[pt], FORM_I32, 0, 0);
    return pt;
}

static int emit_input(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    Tensor& o = net->tensors[net->nodes[i].out];
    st.kind = S_INPUT;
    if (o.forms.empty()) add_form(o, FORM_I32, 0, 0);
    // int8 formats that need a real shift (quant_input=1 on the network input) go through the
    // int32 form + a stand-alone requant; the n == 0 format is a plain narrowing in the input kernel
    for (size_t f = 0; f < o.forms.size(); ++f)
        if (o.forms[f].kind == FORM_I8 && o.forms[f].n != 0) extra->push_back((int)f);
    if (!extra->empty()) add_form(o, FORM_I32, 0, 0);
    st.out.t = net->nodes[i].out;
    st.name = "input";
    double b = (double)o.C * o.H * o.W * 4;
    for (auto& F : o.forms) b += (double)o.H * o.W * (F.kind == FORM_I32 ? o.Cs * 4 : (F.kind == FORM_STEM ? 4 : o.Cs));
    st.bytes_per_img = b;
    return F8_OK;
}

// MobileNet-V2 head: 3x3 / 2 conv + depthwise 3x3 + this 1x1 in one launch
static int emit_head2(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors; auto& ND = net->nodes;
    Node& nd = ND[i]; Node& hh = ND[nd.blk.b0]; Node& hb = ND[nd.blk.b2];
    const Tensor& s = T[hh.a];
    st.kind = S_HEAD2;
    st.src_t = hh.a; st.src_f = find_form(s, FORM_STEM, 0, 0);
    pack_conv_weights(net, hh);
    pack_dw_weights(net, hb);
    pack_conv_weights(net, nd);
    select_outputs(net, nd.out, &st.out, extra);
    const Tensor& o = T[nd.out];
    const double cpx = (double)o.H * o.W;
    st.ops_per_img = 2.0 * cpx * (32.0 * hh.cd.cin * 9 + 32.0 * 9 + 32.0 * nd.cd.cout);
    st.valu_per_img = 3.0 * cpx * (32.0 + 32.0 + o.Cs * out_forms8(st));
    st.bytes_per_img = (double)s.H * s.W * 4 + out_bytes(st, o, cpx);      // (int8 outputs only: pass 1h)
    st.bytes_const = 32.0 * 100 + 32.0 * 13 + (double)o.Cs * 36;
    st.name = "head3x3s2+dw3x3+1x1:" + tname(net, hh.out) + "+" + tname(net, hb.out) + "+" + tname(net, nd.out);
    return F8_OK;
}

// ResNet head: stem conv + max-pool in one launch
static int emit_stem_pool(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors;
    Node& nd = net->nodes[i];
    const Node& pl = net->nodes[nd.sp_pool];
    const Tensor& s = T[nd.a]; const Tensor& o = T[pl.out];
    st.kind = S_STEMPOOL;
    st.src_t = nd.a; st.src_f = find_form(s, FORM_STEM, 0, 0);
    st.relu0 = nd.cd.relu;
    pack_conv_weights(net, nd);
    select_outputs(net, pl.out, &st.out, extra);
    const double cpx = (double)T[nd.out].H * T[nd.out].W, opx = (double)o.H * o.W;
    st.ops_per_img = conv_ops(net, nd);
    st.valu_per_img = cpx * nd.cd.cout + 3.0 * opx * o.Cs * out_forms8(st);      // one max per conv value; the requantisation runs on the pooled ones
    st.bytes_per_img = (double)s.H * s.W * 4 + out_bytes(st, o, opx);
    st.bytes_const = weight_bytes(net, nd);
    st.name = "stem7x7s2+maxpool3x3s2:" + tname(net, nd.out) + "+" + tname(net, pl.out);
    return F8_OK;
}

// BasicBlock chain: node i is the second conv of its LAST block
static int emit_bchain(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors; auto& ND = net->nodes;
    const Node& nd = ND[i];
    const std::vector<int>& ch = nd.chain;
    const Block& r0 = ND[ch[0]].blk;
    const bool ds = r0.sc >= 0;                  // the chain starts with the stage-opening block: ch[0] is its shortcut conv
    const Node& f1 = ND[r0.b0];
    const Tensor& x = T[f1.a];
    st.kind = S_BCHAIN;
    if (!ds) { st.src_t = f1.a; st.src_f = find_form(x, FORM_I32, 0, 0); }
    else if (int rc = conv_input_i8(net, f1, &st.src_t, &st.src_f)) return rc;      // its two convs over the block input may read
    else if ((rc = conv_input_i8(net, ND[r0.sc], &st.res_t, &st.res_f))) return rc;  // different int8 forms of it
    for (int h : ch) pack_block(net, ND[h].blk, true, st);
    const int out_t = ND[nd.fused_add].out;
    select_outputs(net, out_t, &st.out, extra);
    const Tensor& o = T[out_t];
    const double px = (double)o.H * o.W;
    st.bytes_per_img = (ds ? (double)x.H * x.W * x.Cs + (st.res_f != st.src_f ? px * x.Cs : 0) : px * x.Cs * 4) + out_bytes(st, o, px);
    st.valu_per_img = (double)ch.size() * px * o.C * (3.0 + 2.0 + 3.0) - 3.0 * px * o.C + 3.0 * px * o.Cs * out_forms8(st);   // per block: first conv's int8, join, the next block's int8 input; the last block's are the output forms
    st.name = "basic_chain_x" + std::to_string(ch.size()) + (ds ? "_ds:" : ":") + tname(net, f1.out) + ".." + tname(net, nd.out);
    return F8_OK;
}

// BasicBlocks of a 7x7 x 512 stage over clusters of eight workgroups (f8_bcchain.hip): node i is the second conv of the LAST block; the first
// block may be the JOIN of the stage-opening block (its shortcut conv hosts it, its body.0 ran in the launch before)
static int emit_bcchain(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors; auto& ND = net->nodes;
    const Node& nd = ND[i];
    const std::vector<int>& ch = nd.chain;
    const Block& r0 = ND[ch[0]].blk;
    const bool tail = r0.sc >= 0;
    st.kind = S_BCHAIN;
    st.cluster = true;
    const Node& f1 = ND[tail ? r0.b2 : r0.b0];
    if (!tail) { st.src_t = f1.a; st.src_f = find_form(T[f1.a], FORM_I32, 0, 0); }
    else if (int rc = conv_input_i8(net, f1, &st.src_t, &st.src_f)) return rc;          // body.0's output in body.2's format
    else if ((rc = conv_input_i8(net, ND[r0.sc], &st.res_t, &st.res_f))) return rc;     // the block input in the shortcut's format
    for (int h : ch) pack_block(net, ND[h].blk, true, st);
    const Tensor& o = T[ND[nd.fused_add].out];               // the stage's output map
    select_outputs(net, pooled_output(net, nd, ND[nd.fused_add].out), &st.out, extra);
    const double px = (double)o.H * o.W, opx = nd.pool >= 0 ? 1.0 : px, n = (double)ch.size();
    st.bytes_per_img = (tail ? px * (T[st.src_t].Cs + T[st.res_t].Cs) : px * o.Cs * 4) + out_bytes(st, o, opx);   // (tail: mid0 + the shortcut's pixels)
    // per block: the first conv's int8 output (the TAIL join has none), the join, the next block's int8 input; the last block's are the output forms
    st.valu_per_img = px * ((n - (tail ? 1 : 0)) * o.C * 3.0 + n * o.C * 2.0 + (n - 1) * o.C * 3.0) + opx * 3.0 * o.Cs * out_forms8(st) + (nd.pool >= 0 ? px * o.C : 0.0);
    st.name = "basic_cluster_chain_x" + std::to_string(ch.size()) + (tail ? "_ds:" : ":") + tname(net, f1.out) + ".." + tname(net, nd.out) + (nd.pool >= 0 ? "+avgpool" : "");
    return F8_OK;
}

// stage chain: node i is the host conv of its LAST block
static int emit_chain(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors; auto& ND = net->nodes;
    const Node& nd = ND[i];
    const std::vector<int>& ch = nd.chain;
    const Block& r0 = ND[ch[0]].blk;
    const bool tail = r0.b0 < 0;                 // first block = the join of a stride-2 opening block (its body.0 + body.2: the S_P12 step in front)
    const bool ds = r0.sc >= 0;                  // ... or a stage-opening block: the chain reads an int8 form of the stage input
    const Node& a0 = ND[tail ? r0.b4 : r0.b0];
    const Tensor& x = T[ND[ds ? r0.sc : r0.b0].a];
    st.kind = S_CHAIN;
    if (!ds) { st.src_t = a0.a; st.src_f = find_form(x, FORM_I32, 0, 0); }
    else if (int rc = conv_input_i8(net, ND[tail ? r0.sc : r0.b0], &st.src_t, &st.src_f)) return rc;    // tail: the shortcut's int8 form
    else if (tail && (rc = conv_input_i8(net, a0, &st.src2_t, &st.src2_f))) return rc;                  // mid2 in body.4's format
    for (int h : ch) pack_block(net, ND[h].blk, true, st);
    const Tensor& o = T[ND[nd.fused_add].out];   // the stage's output map (geometry of the chain)
    select_outputs(net, pooled_output(net, nd, ND[nd.fused_add].out), &st.out, extra);
    const double px = (double)o.H * o.W, opx = nd.pool >= 0 ? 1.0 : px;
    st.bytes_per_img = (tail ? px * (x.Cs + T[st.src2_t].Cs) : px * x.Cs * (ds ? 1 : 4)) + out_bytes(st, o, opx);   // the stage input, once (tail: the shortcut's pixels + mid2)
    // per block: body.0's and body.2's int8 outputs (the TAIL join has none), the join, the next block's int8 input (last block: the output forms)
    const double mid = (double)(tail ? a0.cd.cin : a0.cd.cout);
    st.valu_per_img = px * ((double)(ch.size() - (tail ? 1 : 0)) * 2.0 * mid * 3.0 + (double)ch.size() * o.C * 2.0 + (double)(ch.size() - 1) * o.C * 3.0) +
                      opx * 3.0 * o.Cs * out_forms8(st) + (nd.pool >= 0 ? px * o.C : 0.0);
    st.name = "stage_chain_x" + std::to_string(ch.size()) + (tail ? "_tail" : (ds ? "_ds" : "")) + (nd.pool >= 0 ? "+avgpool:" : ":") + tname(net, a0.out) + ".." + tname(net, nd.out);
    return F8_OK;
}

// fused bottleneck block (node i = body.4), or fused stage-opening block: DS, or the stride-2 opener (node i = the shortcut conv, i.dual = body.4)
static int emit_fused(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors; auto& ND = net->nodes;
    const Node& nd = ND[i];
    const Block& r = nd.blk;
    const Node& na = ND[r.b0]; const Node& nb = ND[r.b2]; const Node& ng = ND[r.b4];
    const bool ds = r.sc >= 0;
    const Tensor& x = T[na.a];                   // (DS: body.0 and the shortcut read one int8 form of it, pass 1d)
    st.kind = S_FUSED;
    st.variant = r.s2 ? V_OPENER : V_BOTTLENECK;
    if (const int rc = conv_input_i8(net, na, &st.src_t, &st.src_f)) return rc;
    pack_block(net, r, false, st);
    if (!ds) { st.res_t = na.a; st.res_f = find_form(x, FORM_I32, 0, 0); }
    join_shifts(T[nd.out].fl - (ds ? T[ng.out].fl : x.fl), &st.acc_shl, &st.res_shl);     // DS: > 0: body.4's result shifts left
    const int out_t = join_output(net, nd, st);
    select_outputs(net, out_t, &st.out, extra);
    const Tensor& o = T[out_t];
    const double px = (double)x.H * x.W, pxo = (double)o.H * o.W;   // stride-2 opener: body.0 runs on the input map
    st.valu_per_img = 3.0 * (px * na.cd.cout + pxo * nb.cd.cout) + pxo * o.C * 2.0 + 3.0 * pxo * o.Cs * out_forms8(st);
    st.bytes_per_img = px * x.Cs * (ds ? 1 : 1 + 4) + out_bytes(st, o, pxo);                // int8 input (identity: + int32 residual), once each
    st.name = std::string(!ds ? "fused_bottleneck_R" : r.s2 ? "fused_opener_s2_R" : "fused_bottleneck_ds_R") + std::to_string(r.R) + ":" +
              block_names(net, r);
    return F8_OK;
}

// 1x1 -> 3x3 of a 7x7 bottleneck block in one launch (node i = the 3x3), or body.0 + body.2 of a stride-2 opening block whose join opens its chain
static int emit_p12(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors;
    Node& nd = net->nodes[i]; Node& na = net->nodes[nd.blk.b0];
    const Tensor& x = T[na.a];
    st.kind = S_P12;
    st.variant = nd.blk.s2 ? V_OPENER : V_P12;
    if (const int rc = conv_input_i8(net, na, &st.src_t, &st.src_f)) return rc;
    pack_conv_weights(net, na);
    pack_conv_weights(net, nd);
    if (st.variant == V_P12) { pack_frag_weights(net, na); pack_frag_weights(net, nd); }      // f8_opener.hip streams the plain [cout][K] images
    st.relu0 = nd.cd.relu;
    select_outputs(net, nd.out, &st.out, extra);
    if (st.out.f32 >= 0) return fail(F8_ERR_UNSUPPORTED, "finalize: the fused 1x1 -> 3x3 launch writes int8 forms only");
    if (st.variant == V_OPENER && (st.out.f8[0] < 0 || st.out.f8[1] >= 0)) return fail(F8_ERR_UNSUPPORTED, "finalize: the stride-2 1x1 -> 3x3 launch writes exactly one int8 form");
    const Tensor& o = T[nd.out];
    const double px = (double)x.H * x.W, pxo = (double)o.H * o.W;
    st.ops_per_img = conv_ops(net, na) + conv_ops(net, nd);
    st.valu_per_img = 3.0 * (px * na.cd.cout + pxo * o.Cs * out_forms8(st));
    st.bytes_per_img = px * x.Cs + out_bytes(st, o, pxo);
    st.bytes_const = weight_bytes(net, na) + weight_bytes(net, nd);
    st.name = std::string(st.variant == V_OPENER ? "fused_opener_s2_p12_R" + std::to_string(nd.blk.R) + ":" : "fused_p12:") + tname(net, na.out) + "+" + tname(net, nd.out);
    return F8_OK;
}

// inverted-residual chain: node i is the project conv of its LAST block
static int emit_irchain(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors; auto& ND = net->nodes;
    const Node& nd = ND[i];
    const std::vector<int>& ch = nd.chain;
    const Node& fa = ND[ND[ch[0]].blk.b0];
    const Tensor& x = T[fa.a];
    st.kind = S_IRCHAIN;
    if (const int rc = conv_input_i8(net, fa, &st.src_t, &st.src_f)) return rc;
    if (ND[ch[0]].fused_add >= 0) { st.res_t = fa.a; st.res_f = find_form(x, FORM_I32, 0, 0); }
    const double px = (double)x.H * x.W;
    double valu = 0;
    std::string blocks;
    for (size_t k = 0; k < ch.size(); ++k) {
        const Node& c = ND[ch[k]];
        const Block& r = c.blk;
        pack_block(net, r, false, st);
        const int bo = c.fused_add >= 0 ? ND[c.fused_add].out : c.out;
        valu += 3.0 * px * (ND[r.b0].cd.cout + ND[r.b2].cd.cout) + (c.fused_add >= 0 ? 2.0 * px * T[bo].C : 0.0) + (k + 1 < ch.size() ? 3.0 * px * T[bo].Cs : 0.0);
        const std::string& lb = T[bo].label;
        blocks += (k ? "+" : "") + (lb.empty() ? tname(net, bo) : lb.substr(0, lb.find('.')));
    }
    const int out_t = join_output(net, nd, st);
    st.relu0 = nd.cd.relu;
    select_outputs(net, out_t, &st.out, extra);
    const Tensor& o = T[out_t];
    st.bytes_per_img = px * x.Cs + (st.res_t >= 0 ? px * x.Cs * 4 : 0) + out_bytes(st, o, px);
    st.valu_per_img = valu + 3.0 * px * o.Cs * out_forms8(st);
    st.name = "ir_chain_x" + std::to_string(ch.size()) + ":" + blocks;
    return F8_OK;
}

// fused inverted residual: node i is the project conv.  B_IR: around a depthwise 3x3 (f8_ir.hip); B_IRK: around a 5x5 / 7x7 (f8_irk.hip)
static int emit_ir(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors; auto& ND = net->nodes;
    const Node& nd = ND[i];
    const Block& r = nd.blk;
    const Node& na = ND[r.b0]; const Node& nb = ND[r.b2];
    const Tensor& x = T[na.a];
    st.kind = r.kind == B_IRK ? S_IRK : S_IR;
    if (const int rc = conv_input_i8(net, na, &st.src_t, &st.src_f)) return rc;
    pack_block(net, r, false, st);
    st.relu0 = nd.cd.relu;
    const int out_t = join_output(net, nd, st);
    if (nd.fused_add >= 0) {
        st.res_t = na.a; st.res_f = find_form(x, FORM_I32, 0, 0);
        join_shifts(T[nd.out].fl - x.fl, &st.acc_shl, &st.res_shl);
    }
    select_outputs(net, out_t, &st.out, extra);
    const Tensor& o = T[out_t];
    const double px = (double)x.H * x.W, pxo = (double)o.H * o.W;
    st.valu_per_img = 3.0 * (px * na.cd.cout + pxo * nb.cd.cout) + (st.res_t >= 0 ? 2.0 * pxo * o.C : 0.0) + 3.0 * pxo * o.Cs * out_forms8(st);
    st.bytes_per_img = px * x.Cs + (st.res_t >= 0 ? px * x.Cs * 4 : 0) + out_bytes(st, o, pxo);
    const std::string tile = r.G > 1 ? "G" + std::to_string(r.G) : "R" + std::to_string(r.R);
    st.name = (st.kind == S_IRK ? "fused_irk" + std::to_string(nb.cd.kernel) : std::string("fused_ir")) + "_s" + std::to_string(nb.cd.stride) + "_" + tile + ":" + block_names(net, r);
    return F8_OK;
}

// depthwise-separable block: node i is the 1x1 conv.  On f8_dws.hip, or (Block::I7, 1k) on a 7 x 7 output map on f8_dws7.hip, with the average pool
// behind it where the plan folds it in
static int emit_dws(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors; auto& ND = net->nodes;
    Node& nd = ND[i];
    const Block& r = nd.blk;
    Node& nb = ND[r.b0];
    const Tensor& x = T[nb.a];
    const bool d7 = r.I7 > 0, pool = nd.pool >= 0;      // (pool: only 1k's blocks)
    st.kind = d7 ? S_DWS7 : S_DWS;
    if (const int rc = conv_input_i8(net, nb, &st.src_t, &st.src_f)) return rc;
    pack_dw_weights(net, nb);
    pack_conv_weights(net, nd);
    pack_frag_weights(net, nd);
    st.relu0 = nd.cd.relu;
    const int out_t = pooled_output(net, nd, nd.out);
    select_outputs(net, out_t, &st.out, extra);
    if (!pool && (st.out.f32 >= 0 || st.out.f8[0] < 0)) return fail(F8_ERR_UNSUPPORTED, "finalize: the depthwise-separable launch writes int8 forms of the block output only");
    const Tensor& o = T[out_t]; const Tensor& y = T[nd.out];
    const double px = (double)x.H * x.W, pxo = (double)y.H * y.W, outpix = pool ? 1.0 : pxo;
    st.ops_per_img = conv_ops(net, nb) + conv_ops(net, nd);
    if (!d7) st.valu_per_img = 3.0 * pxo * (nb.cd.cout + o.Cs * out_forms8(st));      // both requantisations
    // f8_dws7.hip: the depthwise requantisation, one v_dot4 per four taps (a VALU depthwise conv, as emit_conv counts it), the pool's adds, the output forms
    else st.valu_per_img = 3.0 * pxo * nb.cd.cout + 9.0 * pxo * nb.cd.cout / 4.0 + (pool ? pxo * y.C : 0.0) + 3.0 * outpix * o.Cs * out_forms8(st);
    st.bytes_per_img = px * x.Cs + out_bytes(st, o, outpix);
    st.bytes_const = weight_bytes(net, nb) + weight_bytes(net, nd);
    st.name = (d7 ? "fused_dws7:" : "fused_dws:") + block_names(net, r) + (pool ? "+" + tname(net, out_t) : "");
    return F8_OK;
}

// The kernel of a plain conv step (not depthwise), once its inputs and outputs are known; the first that applies, in this order.
static Variant conv_variant(const f8_net* net, const Node& nd, const Step& st, int max_batch) {
    const Options& opt = net->opt;
    const f8_conv_desc& d = nd.cd;
    const Tensor& s = net->tensors[nd.a]; const Tensor& o = net->tensors[nd.out];
    if (st.dense) return V_FC;                   // the classifier: logits straight into the caller's buffer (f8_fc.hip)
    if (nd.pool >= 0) return V_POOL;             // ... and the average pool behind the last 1x1 conv (1i)
    const bool plain = !nd.stem && d.groups == 1;
    if (nd.dil > 1 || nd.rect) return V_IGEMM;   // a dilated or rectangular conv: conv_igemm_kernel walks its taps at any spacing, the LDS-patch / register-weight 3x3 kernels do not
    // the stride-2 3x3 of a late stage-opening block, int8 outputs only: input patch in LDS, weights straight to registers
    if (opt.s2wreg && plain && d.kernel == 3 && d.stride == 2 && d.pad == 1 && nd.fused_add < 0 && nd.dual < 0 && st.out.f32 < 0 && nd.ck == d.cin &&
        s.H == 2 * o.H && s.W == 2 * o.W && conv3x3s2_wreg_supported(nd.ck, o.H, o.W, nd.coutP)) return V_S2WREG;
    // 1x1 convs (plain, with the residual join, or as the dual GEMM of a stage-opening block) whose weight slice per wave
    // fits the register file: weight-stationary kernel, when a launch gives every workgroup a few pixel tiles to walk
    if (opt.wstat && plain && d.kernel == 1 && d.pad == 0) {
        const Node* g = nd.dual >= 0 ? &net->nodes[nd.dual] : nullptr;
        const int k1 = g ? g->ktot : 0;
        if ((!g || (g->cd.kernel == 1 && g->cd.pad == 0 && g->cd.groups == 1)) && conv1x1_wstat_supported(nd.ck, k1, nd.coutP, st.res_t >= 0)) {
            const int imgs = opt.whole_batch_launches ? max_batch : std::max(1, max_batch / opt.split);
            const long tiles = ((long)imgs * ((long)o.H * o.W) + 31) / 32;
            const int ngroups = nd.coutP / (32 * conv1x1_wstat_waves(nd.ck, k1));
            const int cus = net->num_cu > 0 ? net->num_cu : 256;
            if (tiles >= (long)opt.wstat_min_tiles * std::max(1, cus / ngroups)) return V_WSTAT;
        }
    }
    // late, weight-heavy 1x1 convs with int8 outputs only: weights straight to registers (f8_wreg.hip)
    if (opt.wreg && plain && d.kernel == 1 && d.stride == 1 && d.pad == 0 && nd.fused_add < 0 && nd.dual < 0 && st.out.f32 < 0 &&
        conv1x1_wreg_supported(nd.ck, nd.coutP)) return V_WREG;
    return nd.p3_R > 0 ? V_PATCH3X3 : V_IGEMM;
}
// the conv kernels that read the weights in MFMA-fragment order (pack_frag_weights)
static bool reads_frag_weights(Variant v) { return v == V_FC || v == V_POOL || v == V_WSTAT || v == V_S2WREG || v == V_WREG; }

// The tiles f8_net_autotune times on a conv_igemm_kernel step and option igemm_tile (1 .. 4) forces, and which of them a node has an instance for.
static const int kIgemmCandBm[4] = {128, 128, 64, 64}, kIgemmCandBn[4] = {128, 64, 128, 64};
static bool igemm_tile_admissible(const Node& nd, const ConvTile& t) {
    if (t.bn > 64 && nd.coutP <= 64) return false;
    if (nd.dual >= 0 && !(t.bn == 64 || (t.bn == 128 && t.bm == 128))) return false;     // dual-GEMM instances
    if (t.bm == 64 && t.bn == 32) return false;
    return true;
}

// a conv / linear / depthwise conv of its own, with its residual join or dual GEMM and the average pool behind it
static int emit_conv(f8_net* net, int i, int max_batch, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors; auto& ND = net->nodes;
    const Options& opt = net->opt;
    Node& nd = ND[i];
    const f8_conv_desc& d = nd.cd;
    const Tensor& s = T[nd.a];
    st.kind = nd.depthwise ? S_DW : S_CONV;
    if (nd.stem) { st.src_t = nd.a; st.src_f = find_form(s, FORM_STEM, 0, 0); }
    else if (const int rc = conv_input_i8(net, nd, &st.src_t, &st.src_f)) return rc;
    st.relu0 = d.relu;
    if (nd.depthwise) { if (dw_general(nd)) pack_dwk_weights(net, nd); else pack_dw_weights(net, nd); }
    else {
        pack_conv_weights(net, nd);
        const int M1 = T[nd.out].H * T[nd.out].W;
        if (!pick_conv_tile(M1 * max_batch, nd.coutP, nd.ck, nd.fused_add >= 0, opt.bk128 != 0, &nd.tile))
            return fail(F8_ERR_UNSUPPORTED, "finalize: no conv kernel instance for ck=%d coutP=%d", nd.ck, nd.coutP);
        if (nd.dual >= 0) {       // the dual-GEMM instances: 128x64 / 64x64, or 128x128 where many cout tiles re-read X
            const int wide = opt.dual_wide;   // measured: 7x7x2048 join 67 -> 52 us; 14x14x1024 and 28x28x512 are slower with the wide tile
            nd.tile.bk = 64;
            if (nd.coutP >= wide && nd.tile.bm == 128) nd.tile.bn = 128; else nd.tile.bn = 64;
        }
        if (opt.igemm_tile > 0) {     // tests and tuning: one of autotune's candidates where it is admissible (bk stays)
            ConvTile t = nd.tile; t.bm = kIgemmCandBm[opt.igemm_tile - 1]; t.bn = kIgemmCandBn[opt.igemm_tile - 1];
            if (igemm_tile_admissible(nd, t)) nd.tile = t;
        }
        if (!nd.stem && d.groups == 1 && d.kernel == 3 && nd.dil == 1 && d.stride == 1 && d.pad == 1 && nd.ck == d.cin && opt.patch3x3 &&
            !conv3x3_patch_config(d.cin, s.H, s.W, nd.coutP, &nd.p3_R, &nd.p3_imgs, &nd.p3_bn)) nd.p3_R = 0;
    }
    const int join_t = join_output(net, nd, st);
    if (nd.fused_add >= 0) {
        const int other = join_other(net, nd);
        if (nd.dual >= 0) {
            if (const int rc = conv_input_i8(net, ND[nd.dual], &st.src2_t, &st.src2_f)) return rc;
            pack_conv_weights(net, ND[nd.dual]);
        } else {
            st.res_t = other; st.res_f = find_form(T[other], FORM_I32, 0, 0);
        }
        join_shifts(T[nd.out].fl - T[other].fl, &st.acc_shl, &st.res_shl);     // > 0: the residual shifts left
    }
    const int out_t = pooled_output(net, nd, join_t);      // (... and the average pool, 1i)
    const Tensor& o = T[out_t];
    if (o.dense_out) { st.dense = true; st.out.t = out_t; }
    else select_outputs(net, out_t, &st.out, extra);
    if (!nd.depthwise) st.variant = conv_variant(net, nd, st, max_batch);
    const Node* g = nd.dual >= 0 ? &ND[nd.dual] : nullptr;
    const double opix = (double)T[nd.out].H * T[nd.out].W, outpix = nd.pool >= 0 ? 1.0 : opix;
    st.ops_per_img = conv_ops(net, nd) + (g ? conv_ops(net, *g) : 0.0);
    double b = (double)s.H * s.W * (nd.stem ? 4 : s.Cs);            // input once
    if (st.res_t >= 0) b += opix * o.Cs * 4;
    if (g) b += (double)T[g->a].H * T[g->a].W * T[g->a].Cs;
    if (st.dense) b += (double)d.cout * 4;
    st.bytes_per_img = b + out_bytes(st, o, outpix);
    st.valu_per_img = ((st.res_t >= 0 || g) ? 2.0 * opix * o.C : 0.0) + (nd.pool >= 0 ? opix * o.C : 0.0) + 3.0 * outpix * o.Cs * out_forms8(st) + (nd.depthwise ? (double)(geom_of(nd).kh * geom_of(nd).kw) * opix * d.cout / 4.0 : 0.0);   // (a VALU depthwise conv: one v_dot4 per four taps)
    st.bytes_const = weight_bytes(net, nd) + (g ? weight_bytes(net, *g) : 0.0);
    label_conv_step(net, st, nd);
    if (reads_frag_weights(st.variant)) pack_frag_weights(net, nd);
    if (st.variant == V_WSTAT && g) pack_frag_weights(net, ND[nd.dual]);
    return F8_OK;
}

// Which grouped convs run on gconv3x3_kernel (f8_gconv.hip) under option grouped = 1; every other accepted one — and all of them under grouped = 2 — is
// the dense expansion: emit_conv's plain path over block-diagonal weights (pack_conv_weights), slower by cin / cg.  Measured on the seven grouped layers
// of ResNeXt-50 32x4d at 128 images (profiles/gconv_r07.md): the kernel is 1.9x (128 x 56 x 56, cg 4: 51.3 against 98.7 us) to 8.1x (1024 x 14 x 14 / 2,
// cg 32: 15.5 against 126.0 us) faster than the expansion, on every shape — none of its set is routed to the expansion.
static bool gconv_kernel_applies(const Options& opt, const Node& n) {
    const f8_conv_desc& d = n.cd;
    const int cg = d.cin / d.groups;
    return opt.grouped == 1 && d.kernel == 3 && n.dil == 1 && (d.stride == 1 || d.stride == 2) && d.pad <= 1 && d.cin == d.cout && cg >= 2 && cg <= 32 && 32 % cg == 0;
}
// a grouped 3x3 on the slice-diagonal kernel: always a launch of its own, no join
static int emit_gconv(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors;
    Node& nd = net->nodes[i];
    const f8_conv_desc& d = nd.cd;
    const Tensor& s = T[nd.a]; const Tensor& o = T[nd.out];
    st.kind = S_GCONV;
    if (const int rc = conv_input_i8(net, nd, &st.src_t, &st.src_f)) return rc;
    st.relu0 = d.relu;
    pack_gconv_weights(net, nd);
    select_outputs(net, nd.out, &st.out, extra);
    const double opix = (double)o.H * o.W;
    st.ops_per_img = conv_ops(net, nd);
    st.bytes_per_img = (double)s.H * s.W * s.Cs + out_bytes(st, o, opix);
    st.bytes_const = weight_bytes(net, nd);
    st.valu_per_img = 3.0 * opix * o.Cs * out_forms8(st);
    char buf[64]; snprintf(buf, sizeof buf, "gconv3x3s%d:", d.stride);
    st.name = buf + tname(net, nd.out);
    return F8_OK;
}

// a transposed conv (stride >= 2): always a launch of its own on deconv_kernel (f8_deconv.hip), no join
static int emit_deconv(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors;
    Node& nd = net->nodes[i];
    const f8_conv_desc& d = nd.cd;
    const Tensor& s = T[nd.a]; Tensor& o = T[nd.out];
    st.kind = S_DECONV;
    if (const int rc = conv_input_i8(net, nd, &st.src_t, &st.src_f)) return rc;
    st.relu0 = d.relu;
    pack_deconv_weights(net, nd);
    select_outputs_or_i32(net, nd.out, &st.out, extra);
    const double ipx = (double)s.H * s.W, opx = (double)o.H * o.W;
    st.ops_per_img = 2.0 * ipx * d.kernel * d.kernel * d.cin * d.cout;      // every input pixel meets every tap once (what lands outside the output is cropped)
    st.bytes_per_img = ipx * s.Cs + out_bytes(st, o, opx);                  // input once + the output forms
    st.bytes_const = (double)nd.coutP * (nd.ktot + 4);
    st.valu_per_img = 3.0 * opx * o.Cs * out_forms8(st);
    char buf[64]; snprintf(buf, sizeof buf, "deconv%dx%ds%d:", d.kernel, d.kernel, d.stride);
    st.name = buf + tname(net, nd.out);
    return F8_OK;
}

// the launch of conv node i: the chain whose last block it hosts, else the block it hosts, else a conv of its own
static int emit_conv_family(f8_net* net, int i, int max_batch, Step& st, std::vector<int>* extra) {
    static int (*const emit_chain_kind[])(f8_net*, int, Step&, std::vector<int>*) = {nullptr, emit_chain, emit_bchain, emit_bcchain, emit_irchain};   // by ChainKind
    const Node& nd = net->nodes[i];
    if (nd.sp_pool >= 0 && nd.stem) return emit_stem_pool(net, i, st, extra);      // (the ResNet head: a pairwise link, no block)
    if (nd.chain_into == i) return emit_chain_kind[nd.chain_kind](net, i, st, extra);
    switch (nd.blk.kind) {
        case B_HEAD2: return emit_head2(net, i, st, extra);
        case B_BOTTLENECK: case B_OPENING: return emit_fused(net, i, st, extra);
        case B_P12: return emit_p12(net, i, st, extra);
        case B_IR: case B_IRK: return emit_ir(net, i, st, extra);
        case B_DWS: return emit_dws(net, i, st, extra);
        default:
            if (nd.grouped && gconv_kernel_applies(net->opt, nd)) return emit_gconv(net, i, st, extra);
            return emit_conv(net, i, max_batch, st, extra);
    }
}

static int emit_add(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors;
    const Node& nd = net->nodes[i];
    st.kind = S_ADD;
    st.src_t = nd.a; st.src_f = find_form(T[nd.a], FORM_I32, 0, 0);
    st.res_t = nd.b; st.res_f = find_form(T[nd.b], FORM_I32, 0, 0);
    join_shifts(T[nd.a].fl - T[nd.b].fl, &st.acc_shl, &st.res_shl);
    st.relu1 = nd.relu;
    select_outputs(net, nd.out, &st.out, extra);
    st.name = "add:" + tname(net, nd.out);
    const Tensor& o = T[nd.out];
    st.bytes_per_img = (double)o.H * o.W * o.Cs * 8 + out_bytes(st, o, (double)o.H * o.W);
    return F8_OK;
}

static int emit_maxpool(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors;
    const Node& nd = net->nodes[i];
    const Tensor& s = T[nd.a]; Tensor& o = T[nd.out];
    st.kind = S_MAXPOOL;
    st.src_t = nd.a;
    const bool i8 = (o.forms.size() == 1 && o.forms[0].kind == FORM_I8);
    st.src_f = i8 ? find_form(s, FORM_I8, o.forms[0].n, o.forms[0].sgn) : find_form(s, FORM_I32, 0, 0);
    select_outputs_or_i32(net, nd.out, &st.out, extra);
    st.name = std::string(i8 ? "maxpool_i8:" : "maxpool_i32:") + tname(net, nd.out);
    st.bytes_per_img = (double)s.H * s.W * s.Cs * (i8 ? 1 : 4) + out_bytes(st, o, (double)o.H * o.W);
    return F8_OK;
}

static int emit_avgpool(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors;
    const Node& nd = net->nodes[i];
    const Tensor& s = T[nd.a]; Tensor& o = T[nd.out];
    st.kind = S_AVGPOOL;
    st.src_t = nd.a; st.src_f = find_form(s, FORM_I32, 0, 0);
    select_outputs_or_i32(net, nd.out, &st.out, extra);
    st.name = "avgpool_sum:" + tname(net, nd.out);
    st.bytes_per_img = (double)s.H * s.W * s.Cs * 4 + (double)o.Cs * 5;
    return F8_OK;
}

// What a gather step reads (Step::cat_t / cat_f), st.out chosen: in bytes mode every source in the format of each int8 output form, shifted by
// fl_ref - fl_i as pass 2 asked for it (ask_sources); else the sources' int32 forms.
static int select_sources(f8_net* net, Step& st, const std::vector<int>& srcs, int fl_ref, bool bytes_mode, const char* op) {
    const auto& T = net->tensors;
    st.cat_t = srcs;
    if (!bytes_mode)
        for (int x : srcs) st.cat_f[0].push_back(find_form(T[x], FORM_I32, 0, 0));
    for (int k = 0; bytes_mode && k < 2; ++k) {
        if (st.out.f8[k] < 0) continue;
        const Form& F = T[st.out.t].forms[st.out.f8[k]];
        for (int x : srcs) {
            const int f = find_form(T[x], FORM_I8, F.n - (fl_ref - T[x].fl), F.sgn);
            if (f < 0) return fail(F8_ERR_STATE, "f8_net_finalize: planner bug: %s source t%d lacks the output's int8 form", op, x);
            st.cat_f[k].push_back(f);
        }
    }
    return F8_OK;
}

static int emit_concat(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    const Node& nd = net->nodes[i];
    const Tensor& o = net->tensors[nd.out];
    st.kind = S_CONCAT;
    select_outputs_or_i32(net, nd.out, &st.out, extra);
    if (const int rc = select_sources(net, st, nd.srcs, o.fl, nd.bytes_mode, "concat")) return rc;
    const double px = (double)o.H * o.W;
    if (nd.bytes_mode) {
        st.bytes_per_img = 2.0 * px * o.C * out_forms8(st);      // every real byte read once and written once, per form
    } else {
        st.bytes_per_img = px * o.C * 4 + out_bytes(st, o, px);
        st.valu_per_img = px * o.C * (2 + 3 * out_forms8(st));   // align + clamp per value, 3 per int8 value produced
    }
    st.name = (nd.bytes_mode ? "concat_i8:" : "concat_i32:") + tname(net, nd.out);
    return F8_OK;
}

static int emit_upsample(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    const Node& nd = net->nodes[i];
    const Tensor& s = net->tensors[nd.a]; const Tensor& o = net->tensors[nd.out];
    st.kind = S_UPSAMPLE;
    select_outputs_or_i32(net, nd.out, &st.out, extra);
    if (const int rc = select_sources(net, st, {nd.a}, s.fl, nd.bytes_mode, "upsample")) return rc;
    const double ipx = (double)s.H * s.W, opx = (double)o.H * o.W;
    const bool bil = nd.up_mode == F8_UP_BILINEAR;
    if (nd.bytes_mode) {
        st.bytes_per_img = (ipx + opx) * o.C * out_forms8(st);      // every real byte read once and written once, per form
    } else {
        st.bytes_per_img = ipx * o.C * 4 + out_bytes(st, o, opx);
        st.valu_per_img = opx * o.C * ((bil ? 4 : 0) + 3 * out_forms8(st));      // bilinear: one multiply + three multiply-adds per value; 3 per int8 value produced
    }
    st.name = (bil ? "upsample_bilinear_i32:" : nd.bytes_mode ? "upsample_nearest_i8:" : "upsample_nearest_i32:") + tname(net, nd.out);
    return F8_OK;
}

// slice / channel shuffle; a shuffle fused with its concat (Node::cm_cat) reads the concat's operands
static int emit_chanmap(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    const Node& nd = net->nodes[i];
    const Tensor& o = net->tensors[nd.out];
    const bool fused = nd.cm_cat >= 0;
    st.kind = S_CHANMAP;
    select_outputs_or_i32(net, nd.out, &st.out, extra);
    const std::vector<int> srcs = fused ? net->nodes[nd.cm_cat].srcs : std::vector<int>{nd.a};
    if (const int rc = select_sources(net, st, srcs, net->tensors[nd.a].fl, nd.bytes_mode, "slice / shuffle")) return rc;
    const double px = (double)o.H * o.W;
    if (nd.bytes_mode) {
        st.bytes_per_img = 2.0 * px * o.C * out_forms8(st);      // every real byte read once and written once, per form
    } else {
        st.bytes_per_img = px * o.C * 4 + out_bytes(st, o, px);
        st.valu_per_img = px * o.C * 3 * out_forms8(st);         // 3 per int8 value produced
    }
    char tok[48];
    if (nd.kind == N_SLICE) snprintf(tok, sizeof tok, "slice_%s:", nd.bytes_mode ? "i8" : "i32");
    else snprintf(tok, sizeof tok, "%sshuffle%d_%s:", fused ? "concat+" : "", nd.cm_groups, nd.bytes_mode ? "i8" : "i32");
    st.name = tok + tname(net, nd.out);
    return F8_OK;
}

// depth_to_space / space_to_depth
static int emit_pixmap(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    const Node& nd = net->nodes[i];
    const Tensor& o = net->tensors[nd.out];
    st.kind = S_PIXMAP;
    select_outputs_or_i32(net, nd.out, &st.out, extra);
    if (const int rc = select_sources(net, st, {nd.a}, net->tensors[nd.a].fl, nd.bytes_mode, "depth_to_space / space_to_depth")) return rc;
    const double px = (double)o.H * o.W;
    if (nd.bytes_mode) {
        st.bytes_per_img = 2.0 * px * o.C * out_forms8(st);      // every real byte read once and written once, per form
    } else {
        st.bytes_per_img = px * o.C * 4 + out_bytes(st, o, px);
        st.valu_per_img = px * o.C * 3 * out_forms8(st);         // 3 per int8 value produced
    }
    char tok[48];
    snprintf(tok, sizeof tok, "%s%d%s_%s:", nd.kind == N_S2D ? "s2d" : "d2s", nd.pm_block, nd.pm_order == F8_ORDER_CRD ? "crd" : "dcr", nd.bytes_mode ? "i8" : "i32");
    st.name = tok + tname(net, nd.out);
    return F8_OK;
}

// 256 bytes per int8 output form of `forms8` appended to the weight image: the entries requantised to each form (compose_byte_table).  Returns the offset.
static size_t pack_byte_tables(f8_net* net, const std::vector<int32_t>& table, const Requant* r, int nr) {
    const size_t off = round_up_z(net->wblob.size(), 256);
    net->wblob.resize(off + 256 * (size_t)std::max(nr, 1), 0);
    for (int k = 0; k < nr; ++k) compose_byte_table(table.data(), r[k], net->wblob.data() + off + 256 * (size_t)k);
    return off;
}

// f8_net_mul; a hard gate fused into it (Node::mul_gate) makes the launch read the gate's int32 source as its b
static int emit_mul(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors;
    const Node& nd = net->nodes[i];
    const Tensor& A = T[nd.a]; const Tensor& B = T[nd.b]; const Tensor& o = T[nd.out];
    const bool fused = nd.mul_gate >= 0, bcast = B.H * B.W != A.H * A.W, tab = nd.mul_table >= 0;
    st.kind = S_MUL;
    st.src_t = nd.a; st.src_f = find_form(A, FORM_I8, A.fl - nd.md.a_fl, nd.md.a_signed);
    if (fused) { st.res_t = net->nodes[nd.mul_gate].a; st.res_f = find_form(T[st.res_t], FORM_I32, 0, 0); }
    else if (tab) {
        const Node& tn = net->nodes[nd.mul_table];
        st.res_t = tn.a; st.res_f = find_form(T[tn.a], FORM_I8, T[tn.a].fl - tn.td.in_fl, tn.td.in_signed);
        const Requant rb = Requant::of(B.fl - nd.md.b_fl, nd.md.b_signed != 0);
        net->nodes[i].tab_off = pack_byte_tables(net, tn.table, &rb, 1);
    }
    else { st.res_t = nd.b; st.res_f = find_form(B, FORM_I8, B.fl - nd.md.b_fl, nd.md.b_signed); }
    if (st.src_f < 0 || st.res_f < 0) return fail(F8_ERR_STATE, "f8_net_finalize: planner bug: an operand of mul t%d lacks its form", nd.out);
    st.relu1 = nd.md.relu;
    select_outputs_or_i32(net, nd.out, &st.out, extra);
    const double px = (double)o.H * o.W, bpx = (double)B.H * B.W;
    st.bytes_per_img = px * o.C + bpx * o.C * (fused ? 4 : 1) + px * o.C * ((st.out.f32 >= 0 ? 4 : 0) + out_forms8(st));      // real bytes, each once
    st.valu_per_img = px * o.C * (1 + (nd.md.relu ? 1 : 0) + 3 * out_forms8(st)) + (fused ? bpx * o.C * 5 : 0);      // the multiply, the ReLU, 3 per int8 value produced; a fused gate: clamp + offset + 3
    char tok[48];
    snprintf(tok, sizeof tok, "%s%s_%s:", fused ? "hgate+" : tab ? "table+" : "", bcast ? "chmul" : "mul", st.out.f32 >= 0 ? "i32" : "i8");
    st.name = tok + tname(net, nd.out);
    return F8_OK;
}

// The int8 output forms of a table_i8: launch in the order their byte tables lie in the weight image: slot j of the image belongs to output k = slot_k[j]
// (emit_table composes in this order, bind_step pairs pointer and format by it: TableArgs::bt[k] goes with q[k])
static int table_slots(const OutSel& o, int slot_k[2]) {
    int n = 0;
    for (int k = 0; k < 2; ++k) if (o.f8[k] >= 0) slot_k[n++] = k;
    return n;
}

// f8_net_table as a launch of its own
static int emit_table(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors;
    Node& nd = net->nodes[i];
    const Tensor& s = T[nd.a]; const Tensor& o = T[nd.out];
    st.kind = S_TABLE;
    st.src_t = nd.a; st.src_f = find_form(s, FORM_I8, s.fl - nd.td.in_fl, nd.td.in_signed);
    if (st.src_f < 0) return fail(F8_ERR_STATE, "f8_net_finalize: planner bug: the source of table t%d lacks its form", nd.out);
    select_outputs_or_i32(net, nd.out, &st.out, extra);
    const bool i8 = nd.bytes_mode && st.out.f32 < 0;
    if (i8) {
        Requant r[2]; int slot_k[2];
        const int nr = table_slots(st.out, slot_k);
        for (int j = 0; j < nr; ++j) { const Form& F = o.forms[st.out.f8[slot_k[j]]]; r[j] = Requant::of(F.n, F.sgn != 0); }
        nd.tab_off = pack_byte_tables(net, nd.table, r, nr);
    } else {
        nd.tab_off = round_up_z(net->wblob.size(), 256);
        net->wblob.resize(nd.tab_off + 1024, 0);
        memcpy(net->wblob.data() + nd.tab_off, nd.table.data(), 1024);
    }
    const double px = (double)o.H * o.W;
    st.bytes_per_img = px * o.C * (1 + (st.out.f32 >= 0 ? 4 : 0) + out_forms8(st));
    st.bytes_const = i8 ? 256 * out_forms8(st) : 1024;
    st.valu_per_img = i8 ? 0 : px * o.C * 3 * out_forms8(st);      // bytes mode: a gather, no arithmetic; else 3 per int8 value produced
    st.name = (i8 ? "table_i8:" : "table_i32:") + tname(net, nd.out);
    return F8_OK;
}

// f8_net_hard_gate as a launch of its own
static int emit_hgate(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors;
    const Node& nd = net->nodes[i];
    const Tensor& s = T[nd.a]; const Tensor& o = T[nd.out];
    st.kind = S_HGATE;
    st.src_t = nd.a; st.src_f = find_form(s, FORM_I32, 0, 0);
    select_outputs_or_i32(net, nd.out, &st.out, extra);
    const double px = (double)o.H * o.W;
    st.bytes_per_img = px * o.C * (4 + (st.out.f32 >= 0 ? 4 : 0) + out_forms8(st));
    st.valu_per_img = px * o.C * (2 + 3 * out_forms8(st));      // clamp + offset; 3 per int8 value produced
    st.name = "hgate:" + tname(net, nd.out);
    return F8_OK;
}

static int emit_sumpool(f8_net* net, int i, Step& st, std::vector<int>* extra) {
    auto& T = net->tensors;
    const Node& nd = net->nodes[i];
    const Tensor& s = T[nd.a]; Tensor& o = T[nd.out];
    st.kind = S_SUMPOOL;
    st.src_t = nd.a; st.src_f = find_form(s, FORM_I32, 0, 0);
    select_outputs_or_i32(net, nd.out, &st.out, extra);
    const double opx = (double)o.H * o.W;
    st.bytes_per_img = (double)s.H * s.W * s.Cs * 4 + out_bytes(st, o, opx);
    st.valu_per_img = opx * o.C * (nd.sum_k * nd.sum_k - 1 + 3 * out_forms8(st));      // kernel^2 - 1 adds per value; 3 per int8 value produced
    char tok[48];
    snprintf(tok, sizeof tok, "sumpool%dx%ds%d:", nd.sum_k, nd.sum_k, nd.sum_stride);
    st.name = tok + tname(net, nd.out);
    return F8_OK;
}

// the int8 forms of tensor t beyond the two its producer writes: stand-alone requants of its int32 form
static void emit_requants(f8_net* net, int t, const std::vector<int>& extra) {
    for (int f : extra) {
        const Tensor& x = net->tensors[t];
        Step st; st.kind = S_REQUANT; st.node = x.prod;
        st.src_t = t; st.src_f = find_form(x, FORM_I32, 0, 0);
        st.out.t = t; st.out.f8[0] = f;
        st.name = "requant:" + tname(net, t);
        st.bytes_per_img = (double)x.H * x.W * x.Cs * 5;
        net->steps.push_back(st);
    }
}

// the network output's launch, unless the classifier writes the caller's buffer itself
static void emit_output(f8_net* net, int k = 0) {
    const int t = net->outs[k].t;
    const Tensor& x = net->tensors[t];
    if (x.dense_out) return;
    Step st; st.kind = S_OUTPUT; st.node = x.prod; st.out_k = k;
    st.src_t = t; st.src_f = find_form(x, FORM_I32, 0, 0);
    st.name = (k ? "tap:" : "output:") + tname(net, t);
    st.bytes_per_img = (double)x.H * x.W * (x.Cs + x.C) * 4;
    net->steps.push_back(st);
}

// The launch of argmax output k (f8_argmax.hip), directly behind the producer of what it reads.  up < 0: it reads the marked tensor's int32 form.  up >= 0: the
// upsample node that produces the marked tensor and runs inside this launch (Node::argmax_k): it reads the upsample's SOURCE in int32 and stands in the
// upsample's place in the plan.  It writes no tensor (st.out.t < 0), only the caller's buffer.
static void emit_argmax(f8_net* net, int k, int up) {
    const int t = net->outs[k].t, ib = net->outs[k].idx;
    const Tensor& o = net->tensors[t];
    const Node* u = up >= 0 ? &net->nodes[up] : nullptr;
    const int src = u ? u->a : t;
    const Tensor& x = net->tensors[src];
    Step st; st.kind = S_ARGMAX; st.node = u ? up : o.prod; st.out_k = k;
    st.src_t = src; st.src_f = find_form(x, FORM_I32, 0, 0);
    const bool bil = u && u->up_mode == F8_UP_BILINEAR;
    st.name = std::string(u ? (bil ? "upsample_bilinear+" : "upsample_nearest+") : "") + (ib == F8_IDX_U8 ? "argmax_u8:" : "argmax_i32:") + tname(net, t);
    const double opx = (double)o.H * o.W;
    st.bytes_per_img = (double)x.H * x.W * x.Cs * 4 + opx * ib;      // the source's blocks once (the fused launch re-reads them from cache), one index per pixel
    st.valu_per_img = opx * o.C * ((bil ? 4 : 0) + 3);               // bilinear: one multiply + three multiply-adds per value; compare, select the maximum, select the index
    net->steps.push_back(st);
}

// the fused stem launch can read the raw input itself: the input step then launches nothing (run_step)
static void let_stem_read_input(f8_net* net) {
    for (auto& st : net->steps) {
        if (st.kind != S_INPUT) continue;
        const Tensor& o = net->tensors[st.out.t];
        if (!only_stem_form(o) || o.C != 3 || !net->opt.fuse_input) continue;
        Step* stem = nullptr; int users = 0;
        for (auto& s2 : net->steps) {
            if (s2.src_t == st.out.t) { ++users; if (s2.kind == S_STEMPOOL || s2.kind == S_HEAD2) stem = &s2; }
            users += (int)std::count(s2.cat_t.begin(), s2.cat_t.end(), st.out.t);      // a concat that reads the input (it asks for another form: never reached today)
        }
        if (stem && users == 1) {
            st.raw_input = stem->raw_input = true;
            stem->bytes_per_img += (double)o.C * o.H * o.W * 4 - (double)o.H * o.W * 4;      // int32 planes instead of the NHWC4 copy
            st.bytes_per_img = 0;
            st.name = "input(read by the stem launch)";
        }
    }
}

static int emit_steps(f8_net* net, int max_batch) {
    net->steps.clear();
    int taps = 0, amaxes = 0, want_taps = 0, want_amaxes = 0;
    for (size_t k = 0; k < net->outs.size(); ++k) { want_amaxes += net->outs[k].idx != 0; want_taps += k >= 1 && !net->outs[k].idx; }
    for (int i = 0; i < (int)net->nodes.size(); ++i) {
        const Node& nd = net->nodes[i];
        if (nd.kind == N_UPSAMPLE && nd.argmax_k >= 0) { emit_argmax(net, nd.argmax_k, i); ++amaxes; continue; }      // the argmax launch interpolates itself
        if (nd.kind == N_ADD && nd.fused_into >= 0) continue;
        if (nd.kind == N_CONV && (nd.absorbed_by >= 0 || nd.dual_host >= 0)) continue;
        if (nd.kind == N_CONV && nd.chain_into >= 0 && nd.chain_into != i) continue;      // runs inside the chain launch of a later block
        if (nd.kind == N_MAXPOOL && nd.sp_conv >= 0) continue;
        if (nd.kind == N_AVGPOOL && nd.pool_host >= 0) continue;     // runs in its conv's launch
        if (nd.kind == N_CONCAT && nd.cat_into >= 0) continue;       // the shuffle behind it reads its operands
        if (nd.kind == N_HGATE && nd.gate_into >= 0) continue;       // the mul behind it applies it
        if (nd.kind == N_TABLE && nd.tab_into >= 0) continue;        // the mul behind it looks it up
        Step st; st.node = i;
        std::vector<int> extra;
        int rc = F8_OK;
        switch (nd.kind) {
            case N_INPUT: rc = emit_input(net, i, st, &extra); break;
            case N_CONV: case N_LINEAR: rc = emit_conv_family(net, i, max_batch, st, &extra); break;
            case N_ADD: rc = emit_add(net, i, st, &extra); break;
            case N_MAXPOOL: rc = emit_maxpool(net, i, st, &extra); break;
            case N_AVGPOOL: rc = emit_avgpool(net, i, st, &extra); break;
            case N_CONCAT: rc = emit_concat(net, i, st, &extra); break;
            case N_UPSAMPLE: rc = emit_upsample(net, i, st, &extra); break;
            case N_DECONV: rc = emit_deconv(net, i, st, &extra); break;
            case N_SUMPOOL: rc = emit_sumpool(net, i, st, &extra); break;
            case N_SLICE: case N_SHUFFLE: rc = emit_chanmap(net, i, st, &extra); break;
            case N_D2S: case N_S2D: rc = emit_pixmap(net, i, st, &extra); break;
            case N_MUL: rc = emit_mul(net, i, st, &extra); break;
            case N_HGATE: rc = emit_hgate(net, i, st, &extra); break;
            case N_TABLE: rc = emit_table(net, i, st, &extra); break;
        }
        if (rc) return rc;
        net->steps.push_back(st);
        emit_requants(net, st.out.t, extra);
        // a further output leaves directly behind the launch that writes its int32 form: the form's lifetime ends here unless the net reads it
        // again, and the arena reuses its space (at the end of the plan every tapped map would stay allocated through the whole run)
        const int k = output_index(net, st.out.t);
        if (k >= 1) { emit_output(net, k); ++taps; }
        // ... and so does an argmax output, whatever its index (output 0 included: it has no copy-out launch at the end of the plan)
        const int ka = st.out.t >= 0 ? argmax_index(net, st.out.t) : -1;
        if (ka >= 0) { emit_argmax(net, ka, -1); ++amaxes; }
    }
    if (taps != want_taps || amaxes != want_amaxes) return fail(F8_ERR_UNSUPPORTED, "f8_net_finalize: an output tensor is written by no launch of the plan");
    if (!net->outs[0].idx) emit_output(net);
    let_stem_read_input(net);
    return F8_OK;
}

// pass 4
static int layout_arena(f8_net* net, int max_batch) {
    auto& T = net->tensors;
    // ---- 4. lifetimes and arena layout (first-fit over a free list; in-place residual update)
    auto touch = [&](int t, int f, int step) {
        if (t < 0 || f < 0) return;
        Form& F = T[t].forms[f];
        if (F.first < 0) F.first = step;
        F.last = std::max(F.last, step);
    };
    for (size_t si = 0; si < net->steps.size(); ++si) {
        Step& st = net->steps[si];
        touch(st.src_t, st.src_f, (int)si);
        touch(st.res_t, st.res_f, (int)si);
        touch(st.src2_t, st.src2_f, (int)si);
        for (int k = 0; k < 2; ++k)
            for (size_t j = 0; j < st.cat_f[k].size(); ++j) touch(st.cat_t[j], st.cat_f[k][j], (int)si);
        if (st.out.t >= 0 && !st.dense) {
            touch(st.out.t, st.out.f32, (int)si);
            touch(st.out.t, st.out.f8[0], (int)si);
            touch(st.out.t, st.out.f8[1], (int)si);
            if (st.kind == S_INPUT)
                for (size_t f = 0; f < T[st.out.t].forms.size(); ++f) touch(st.out.t, (int)f, (int)si);
        }
    }
    struct Blk { size_t off, size; };
    std::vector<Blk> freel;
    size_t top = 0;
    auto alloc = [&](size_t sz) -> size_t {
        sz = round_up_z(sz, 256);
        size_t best = (size_t)-1; int bi = -1;
        for (size_t i = 0; i < freel.size(); ++i)
            if (freel[i].size >= sz && freel[i].size < best) { best = freel[i].size; bi = (int)i; }
        if (bi >= 0) {
            size_t off = freel[bi].off;
            if (freel[bi].size == sz) freel.erase(freel.begin() + bi);
            else { freel[bi].off += sz; freel[bi].size -= sz; }
            return off;
        }
        size_t off = top; top += sz; return off;
    };
    auto release = [&](size_t off, size_t sz) {
        sz = round_up_z(sz, 256);
        freel.push_back({off, sz});
        std::sort(freel.begin(), freel.end(), [](const Blk& a, const Blk& b) { return a.off < b.off; });
        for (size_t i = 0; i + 1 < freel.size();)
            if (freel[i].off + freel[i].size == freel[i + 1].off) { freel[i].size += freel[i + 1].size; freel.erase(freel.begin() + i + 1); }
            else ++i;
    };
    for (auto& t : T)
        for (auto& F : t.forms) {
            if (F.kind == FORM_I32) { F.bytes_per_img = (size_t)t.H * t.W * t.Cs * 4; F.slack = (size_t)32 * t.Cs * 4; }
            else if (F.kind == FORM_I8) F.bytes_per_img = (size_t)t.H * t.W * t.Cs;
            else F.bytes_per_img = (size_t)F.Hp * F.Wp * 4;
        }
    // the stem image keeps a zero halo that is written once at upload: give it a private region
    for (auto& t : T)
        for (auto& F : t.forms)
            if (F.kind == FORM_STEM) {
                F.off = alloc(F.bytes_per_img * max_batch);
                net->stem_zero_off = F.off; net->stem_zero_bytes = F.bytes_per_img * max_batch;
                net->stem_zero_val = F.sgn ? 0 : 0x80;
            }
    // Chunked execution (for_each_launch) interleaves the steps of a chunk group: chunk c runs steps i..j-1 before chunk c+1
    // does.  A form that dies inside the group is therefore still needed by later chunks while forms born later in the group
    // are already being written by earlier chunks: for the allocator the whole group is ONE step (forms born in it live from
    // its first step, forms dying in it until its last).  Groups are taken as large as any option setting can make them.
    const int ns_all = (int)net->steps.size();
    std::vector<int> gstart(ns_all), gend(ns_all);
    {
        auto chunkable_w = [&](int k) -> int {
            const Step& st = net->steps[k];
            if (st.kind != S_FUSED) return 0;
            const Tensor& x = T[st.src_t];
            return (x.W == x.H && (x.W == 56 || x.W == 28 || x.W == 14)) ? x.W : 0;
        };
        for (int i = 0; i < ns_all;) {
            int j = i + 1;
            const int w = chunkable_w(i);
            if (w) while (j < ns_all && chunkable_w(j) == w) ++j;
            for (int k = i; k < j; ++k) { gstart[k] = i; gend[k] = j - 1; }
            i = j;
        }
    }
    for (int si = 0; si < ns_all; ++si) {
        // forms born at this (super) step, in the order of their producing steps
        if (gstart[si] == si)
            for (int sj = si; sj <= gend[si]; ++sj) {
                Step& st = net->steps[sj];
                for (size_t ti = 0; ti < T.size(); ++ti)
                    for (size_t f = 0; f < T[ti].forms.size(); ++f) {
                        Form& F = T[ti].forms[f];
                        if (F.kind == FORM_STEM || F.first != sj) continue;
                        // in-place residual: out32 of a conv/add step may overwrite a residual operand that dies here
                        // (each thread reads its element before writing it; same geometry, so it also holds per chunk)
                        if (F.kind == FORM_I32 && (int)ti == st.out.t && (int)f == st.out.f32 && st.res_t >= 0 &&
                            (st.kind == S_CONV || st.kind == S_ADD || st.kind == S_FUSED || st.kind == S_IR)) {
                            Form& R = T[st.res_t].forms[st.res_f];
                            if (R.last == sj && R.bytes_per_img == F.bytes_per_img && R.kind == FORM_I32) {
                                F.off = R.off; R.last = -2;   // ownership moves to F
                                continue;
                            }
                        }
                        F.off = alloc(F.bytes_per_img * max_batch + F.slack);
                    }
            }
        // forms dying at this (super) step
        if (gend[si] == si)
            for (size_t ti = 0; ti < T.size(); ++ti)
                for (auto& F : T[ti].forms)
                    if (F.kind != FORM_STEM && F.first >= 0 && F.last >= gstart[si] && F.last <= si) release(F.off, F.bytes_per_img * max_batch + F.slack);
    }
    net->arena_bytes = top;
    for (auto& t : T)
        for (auto& F : t.forms)
            if (F.bytes_per_img * (size_t)max_batch >= (1ull << 31))
                return fail(F8_ERR_UNSUPPORTED, "finalize: a tensor exceeds 2 GiB at max_batch %d (buffer addressing)", max_batch);
    return F8_OK;
}

// ------------------------------------------------------------------------------ bind
// Fills st.args with every launch argument the plan decides: geometry, divisors (FastDiv), consumer formats (Requant), ReLU flags, join shifts, the bounds
// of the float requantisation, output formats; chooses the instance the launcher starts (st.inst: the family's *_inst, f8_internal.h) and
// names it (st.kernel).  Weight pointers are set once the weights are on the device (f8_net_upload binds again).  What a run decides is run_step's.
static int bind_step(f8_net* net, Step& st) {
    auto& T = net->tensors; auto& ND = net->nodes;
    Node& nd = ND[st.node];
    int rc = F8_OK;
    auto W8 = [&](size_t off) { return net->d_w ? (const int8_t*)(net->d_w + off) : nullptr; };
    auto B32 = [&](size_t off) { return (const int32_t*)W8(off); };
    // the int8 input format of conv c: shift from its source tensor, clamp bounds, storage bias (unsigned formats are stored x ^ 0x80)
    auto fmt = [&](const Node& c) {
        int v = 0;
        const int r = consumer_format(T[c.a], c.cd, &v, "finalize");
        if (!rc) rc = r;
        return Requant::of(v, c.cd.input_signed != 0);
    };
    auto out_formats = [&](QuantOut q[2]) {
        if (st.out.t < 0 || st.dense) return;
        for (int k = 0; k < 2; ++k) if (st.out.f8[k] >= 0) set_q(q[k], T[st.out.t].forms[st.out.f8[k]]);
    };
    const int nq = (st.out.t >= 0 && !st.dense) ? (st.out.f8[0] >= 0) + (st.out.f8[1] >= 0) : 0;   // int8 output forms: q[0 .. nq - 1] (select_outputs)
    const bool res = st.res_t >= 0, out32 = st.out.f32 >= 0;
    const int rq_int = !net->opt.requant_float;
    const Options& opt = net->opt;
    // What IRArgs and IRKArgs name alike (block hosted by nd: expand na -> depthwise nb -> project nd; map x -> oT): weights, geometry, formats, join, divisors
    auto bind_ir_common = [&](auto& a, const Node& na, const Node& nb, const Tensor& x, const Tensor& oT) {
        const Block& r = nd.blk;
        a.w0 = W8(na.w_off); a.b0 = B32(na.b_off);
        a.wd4 = W8(nb.rc_off); a.bd4 = B32(nb.cc_off);           // the depthwise conv's dot4 image; bias + 128 * sum(w) for unsigned inputs
        a.w4 = W8(nd.w_off); a.b4 = B32(nd.b_off);
        a.H = x.H; a.W = x.W; a.Ho = oT.H; a.Wo = oT.W; a.stride = nb.cd.stride; a.R = r.R; a.G = r.G; a.E32 = na.coutP;
        a.set_r(fmt(nb), fmt(nd));
        a.relu_a = na.cd.relu; a.relu_b = nb.cd.relu; a.relu0 = st.relu0;
        a.acc_shl = st.acc_shl; a.res_shl = st.res_shl; a.relu1 = st.relu1;
        a.dW = fast_divisor((uint32_t)x.W);
        a.dHW = fast_divisor((uint32_t)(x.H * x.W));
        a.dWo = fast_divisor((uint32_t)oT.W);
        a.dRWo = fast_divisor((uint32_t)(r.R * oT.W));
        out_formats(a.q);
    };
    // ... DwsArgs and Dws7Args (depthwise nb -> 1x1 nd over block input x); the depthwise weights are each case's own image
    auto bind_dws_common = [&](auto& a, Node& nb, const Tensor& x) {
        a.w1 = W8(nd.wf_off); a.b1 = B32(nd.b_off);
        a.H = x.H; a.W = x.W; a.Cin = x.Cs; a.Cout = nd.coutP; a.stride = nb.cd.stride;
        a.in_signed = nb.cd.input_signed;
        a.r1 = fmt(nd);
        a.relu0 = st.relu0;
        a.acc_ok = conv_acc_bounded(nb) && conv_acc_bounded(nd); a.rq_int = rq_int;
        out_formats(a.q);
    };
    // ... and one block of a BasicBlock chain, cluster launch or not, as far as it has a first conv (c1 -> c2, the join hosted by hk): not the opening block's join alone
    auto bind_basic_block = [&](BChainBlk& B, const Node& hk, const Node& c1, const Node& c2) {
        B.wa = W8(c1.wf_off); B.wb = W8(c2.wf_off);
        B.ba = B32(c1.b_off); B.bb = B32(c2.b_off);
        B.rq = fmt(c1);
        B.r1 = fmt(c2);
        B.relu_a = c1.cd.relu; B.relu1 = ND[hk.fused_add].relu;
    };
    char kb[192] = "";
    switch (st.kind) {
        case S_INPUT: {                                   // (its arguments are the run's: run_step)
            const Tensor& o = T[st.out.t];
            st.inst = input_inst(o.C, o.W, only_stem_form(o));
            snprintf(kb, sizeof kb, "%s", input_kernel_name(st.inst));
            break;
        }
        case S_CONV: {
            const Tensor& sT = T[st.src_t]; const Form& sF = sT.forms[st.src_f];
            const Tensor& oT = T[nd.out];
            const f8_conv_desc& d = nd.cd;
            ConvArgs a{};
            a.w = W8(nd.w_off); a.w_bytes = (uint32_t)((size_t)nd.coutP * nd.ktot);
            a.bias = B32(nd.b_off);
            a.PQ = oT.H * oT.W; a.Q = oT.W;
            a.dPQ = fast_divisor((uint32_t)a.PQ);
            a.dQ = fast_divisor((uint32_t)a.Q);
            const f8_conv_geom g = geom_of(nd);           // per axis: the rows by (stride, pad), the columns by (stride_w, pad_w)
            a.stride = g.stride_h; a.stride_w = g.stride_w; a.kh = g.kh; a.CK = nd.ck; a.ktot = nd.ktot; a.coutP = nd.coutP;
            a.ncc = nd.ncc;
            if (nd.ncc > 0) { a.rowcls = (const uint8_t*)W8(nd.rc_off); a.colcls = (const uint8_t*)W8(nd.cc_off); }
            if (nd.stem) {
                a.sN = (int)sF.bytes_per_img; a.sP = d.stride * sF.Wp * 4; a.sQ = d.stride * 4;
                a.origin = 0; a.H = sF.Hp; a.W = sF.Wp; a.pad = 0; a.kw = 1;
                a.tapH = sF.Wp * 4; a.tapW = 0;
            } else {
                a.sN = sT.H * sT.W * sT.Cs; a.sP = g.stride_h * sT.W * sT.Cs; a.sQ = g.stride_w * sT.Cs;
                a.origin = -(g.pad_top * sT.W + g.pad_left) * sT.Cs; a.H = sT.H; a.W = sT.W; a.pad = g.pad_top; a.pad_w = g.pad_left; a.kw = g.kw;
                a.pad_far = std::max(g.pad_bottom, g.pad_right);
                a.tapH = sT.W * sT.Cs; a.tapW = sT.Cs;
            }
            a.dil = nd.stem ? 1 : nd.dil; a.kwd = a.kw * a.dil;     // (conv_igemm_kernel carries its tap coordinates pre-dilated; every other variant is undilated)
            a.relu0 = st.relu0;
            if (st.res_t >= 0 || nd.dual >= 0) { a.acc_shl = st.acc_shl; a.res_shl = st.res_shl; a.relu1 = st.relu1; }
            if (nd.dual >= 0) {
                const Node& g = ND[nd.dual];
                const Tensor& s2 = T[st.src2_t];
                a.w2 = W8(g.w_off); a.w2_bytes = (uint32_t)((size_t)g.coutP * g.ktot);
                a.bias2 = B32(g.b_off);
                a.sN2 = s2.H * s2.W * s2.Cs; a.sP2 = g.cd.stride * s2.W * s2.Cs; a.sQ2 = g.cd.stride * s2.Cs; a.ktot2 = g.ktot;
            }
            // the kernels that read the fragment-order weight image
            if (reads_frag_weights(st.variant)) a.w = W8(nd.wf_off);
            if (st.variant == V_WSTAT && nd.dual >= 0) a.w2 = W8(ND[nd.dual].wf_off);
            out_formats(a.q);
            switch (st.variant) {                         // (run_step: the same cases)
                case V_FC: fc_dense_kernel_name(kb, sizeof kb, a); break;
                case V_POOL: conv1x1_pool_kernel_name(kb, sizeof kb, a, res); break;
                case V_S2WREG: conv3x3s2_wreg_kernel_name(kb, sizeof kb, a); break;
                case V_WSTAT: conv1x1_wstat_kernel_name(kb, sizeof kb, a, st.inst = conv1x1_wstat_inst(a, res, out32, nq, opt.wstat_fast)); break;
                case V_WREG: conv1x1_wreg_kernel_name(kb, sizeof kb, a); break;
                case V_PATCH3X3: conv3x3_patch_kernel_name(kb, sizeof kb, d.cin, a.W, res); break;
                default: conv_kernel_name(kb, sizeof kb, a, nd.tile, st.inst = conv_inst(a, nd.tile, res, nd.dual >= 0, opt.deep_nk));   // V_IGEMM
            }
            st.args = a; break;
        }
        case S_HEAD2: case S_STEMPOOL: {
            const bool h2 = st.kind == S_HEAD2;
            Node& hc = h2 ? ND[nd.blk.b0] : nd;           // the head conv
            const Tensor& sT = T[st.src_t]; const Form& sF = sT.forms[st.src_f];
            StemPoolArgs a{};
            a.w = W8(hc.w_off); a.w_bytes = (uint32_t)((size_t)hc.coutP * hc.ktot);
            a.bias = B32(hc.b_off);
            a.Hp = sF.Hp; a.Wp = sF.Wp; a.org = sF.pad - hc.cd.pad;
            a.raw_kind = -1;
            if (h2) {
                Node& hb = ND[nd.blk.b2];
                const Tensor& oT = T[nd.out];
                a.h2 = head_dws_form(nd) ? 2 : 1;         // 2: head_dws_kernel (pass 1h, option fuse_head_dws)
                a.relu1 = nd.cd.relu ? 1 : 0; a.Cs = oT.Cs;
                a.wd = W8(hb.w_off); a.bd = B32(hb.cc_off);
                a.w1 = W8(nd.w_off); a.b1 = B32(nd.b_off);
                a.na = fmt(hb).n; a.nb = fmt(nd).n;
                a.Pc = oT.H; a.Qc = oT.W; a.P = oT.H; a.Q = oT.W;
                a.relu0 = 1;
                a.acc_ok = conv_acc_bounded(hc) && conv_acc_bounded(hb) && conv_acc_bounded(nd); a.rq_int = rq_int || !a.acc_ok;
                a.rC = sT.C; a.rH = sT.H; a.rW = sT.W; a.xor8 = Requant::of(0, sF.sgn).bias_xor;
            } else {
                const Tensor& cT = T[nd.out]; const Tensor& oT = T[ND[nd.sp_pool].out];
                a.Pc = cT.H; a.Qc = cT.W; a.P = oT.H; a.Q = oT.W;
                a.relu0 = st.relu0;
                a.acc_ok = conv_acc_bounded(nd); a.rq_int = rq_int;
            }
            StemPoolArgs g = a; g.rH = sT.H; g.rW = sT.W;      // (the raw input's sides: run_step binds them where the launch reads it)
            st.inst = stem_pool_inst(g, opt.stem_rows, st.raw_input);
            snprintf(kb, sizeof kb, "%s", stem_pool_kernel_name(st.inst));
            out_formats(a.q); st.args = a; break;
        }
        case S_FUSED: {
            const Block& r = nd.blk;
            const bool ds = r.sc >= 0, opener = st.variant == V_OPENER;     // stage-opening block: nd = shortcut conv, nd.dual = body.4
            const Node& na = ND[r.b0]; const Node& nb = ND[r.b2]; const Node& ng = ND[r.b4];
            const Tensor& x = T[st.src_t];
            FusedArgs a{};
            a.w0 = W8(na.w_off); a.w0_bytes = (uint32_t)((size_t)na.coutP * na.ktot);
            a.w2 = W8(nb.w_off); a.w2_bytes = (uint32_t)((size_t)nb.coutP * nb.ktot);
            a.w4 = W8(ng.w_off); a.w4_bytes = (uint32_t)((size_t)ng.coutP * ng.ktot);
            a.b0 = B32(na.b_off); a.b2 = B32(nb.b_off); a.b4 = B32(ng.b_off);
            if (ds) {
                a.wsc = W8(nd.w_off); a.wsc_bytes = (uint32_t)((size_t)nd.coutP * nd.ktot); a.bsc = B32(nd.b_off);
                a.COUT = nd.cd.cout; a.stride2 = opener ? 1 : 0;
            }
            a.H = x.H; a.W = x.W; a.C = na.cd.cin; a.MID = na.cd.cout; a.R = r.R;
            a.tiles_per_img = opener ? (x.H / 2) / r.R : (x.H + r.R - 1) / r.R;
            a.r1 = fmt(nb);
            a.r2 = fmt(ng);
            a.relu_a = na.cd.relu; a.relu_b = nb.cd.relu;
            a.acc_shl = st.acc_shl; a.res_shl = st.res_shl; a.relu1 = st.relu1;
            out_formats(a.q);
            if (opener) fused_opener_kernel_name(kb, sizeof kb, a, st.inst = fused_opener_inst(a, opt.opener_stg));
            else fused_bottleneck_kernel_name(kb, sizeof kb, a);
            st.args = a; break;
        }
        case S_P12: {
            Node& na = ND[nd.blk.b0];
            const Tensor& x = T[st.src_t];
            FusedArgs a{};
            const bool opener = st.variant == V_OPENER;
            const size_t w0 = opener ? na.w_off : na.wf_off, w2 = opener ? nd.w_off : nd.wf_off;   // f8_p12.hip reads fragment order
            a.w0 = W8(w0); a.w0_bytes = (uint32_t)((size_t)na.coutP * na.ktot);
            a.w2 = W8(w2); a.w2_bytes = (uint32_t)((size_t)nd.coutP * nd.ktot);
            a.b0 = B32(na.b_off); a.b2 = B32(nd.b_off);
            a.H = x.H; a.W = x.W; a.C = na.cd.cin; a.MID = na.cd.cout;
            a.r1 = fmt(nd);
            a.relu_a = na.cd.relu; a.relu_b = nd.cd.relu;
            out_formats(a.q);
            if (opener) {                                 // body.0 + body.2 of a stride-2 opening block on f8_opener.hip (P12); q[0] = mid2
                a.COUT = 4 * na.cd.cout; a.R = nd.blk.R;
                a.tiles_per_img = (x.H / 2 + a.R - 1) / a.R;
                a.r2 = a.q[0];                                // mid2's one form = body.4's input format
                a.stride2 = 1; a.p12only = 1; a.acc_ok = conv_acc_bounded(na) && conv_acc_bounded(nd); a.rq_int = rq_int;
                fused_opener_kernel_name(kb, sizeof kb, a, st.inst = fused_opener_inst(a, opt.opener_stg));
            } else fused_p12_kernel_name(kb, sizeof kb, a);
            st.args = a; break;
        }
        case S_CHAIN: {
            const std::vector<int>& ch = nd.chain;
            ChainArgs a{};
            a.nblk = (int)ch.size();
            unsigned shortcut_blocks = 0;
            for (int k = 0; k < a.nblk; ++k) {
                const Node& hh = ND[ch[k]];
                const Block& r = ND[ch[k]].blk;
                const Node& ng = ND[r.b4];
                ChainBlk& B = a.blk[k];
                B.w4 = W8(ng.wf_off); B.b4 = B32(ng.b_off);
                if (r.sc >= 0) { B.wsc = W8(hh.wf_off); B.bsc = B32(hh.b_off); shortcut_blocks |= 1u << k; }
                B.relu1 = ND[hh.fused_add].relu;
                // identity: (body.4 << acc_shl) + (block input << res_shl); opening block: (shortcut << acc_shl) + (body.4 << res_shl)
                join_shifts(T[hh.out].fl - (r.sc >= 0 ? T[ng.out].fl : T[ND[r.b0].a].fl), &B.acc_shl, &B.res_shl);
                if (r.b0 < 0) {                                 // only the join of a stride-2 opening block (tail: always the first block)
                    B.rq = B.r1 = B.r2 = Requant::of(1, false);    // (unused: no body.0 / body.2 here)
                    B.relu_a = B.relu_b = 1;
                    a.acc_ok = 1; a.stream_ok = stream_bounded(net, ND[hh.fused_add].out) ? 1 : 0; a.rq_int = rq_int;
                    continue;
                }
                Node& na = ND[r.b0]; Node& nb = ND[r.b2];
                B.w0 = W8(na.wf_off); B.w2 = W8(nb.wf_off);
                B.b0 = B32(na.b_off); B.b2 = B32(nb.b_off);
                B.rq = fmt(na);
                B.r1 = fmt(nb);
                B.r2 = fmt(ng);
                B.relu_a = na.cd.relu; B.relu_b = nb.cd.relu;
                if (k == 0) { a.acc_ok = 1; a.rq_int = rq_int; a.stream_ok = (r.sc >= 0 || stream_bounded(net, na.a)) ? 1 : 0; }   // identity first block: the stream it reads
                a.acc_ok = a.acc_ok && conv_acc_bounded(na) && conv_acc_bounded(nb);
                a.stream_ok = a.stream_ok && stream_bounded(net, ND[hh.fused_add].out);
            }
            const Node& hf = ND[ch[0]];
            const Block& r0 = ND[ch[0]].blk;
            const bool tail = r0.b0 < 0, ds = r0.sc >= 0;
            const Node& a0 = ND[tail ? r0.b4 : r0.b0];
            const Tensor& oT = T[ND[nd.fused_add].out];      // the stage's output map (st.out.t: the pooled tensor when the pool runs in the launch)
            a.tail = tail ? 1 : 0;
            a.pool = nd.pool >= 0 ? 1 : 0;
            st.C = oT.C; st.MID = tail ? a0.cd.cin : a0.cd.cout; st.H = oT.H; st.W = oT.W; st.cin0 = tail ? hf.cd.cin : a0.cd.cin;
            chain_shape(st.C, st.MID, st.H, st.W, st.cin0, tail, &a.R, &st.wg_per_cu);
            st.cluster = (!ds || tail) && cchain_supported(st.C, st.MID, st.H, st.W, st.cin0, tail);   // the 7x7 stage: clusters of eight workgroups
            // option chain_stack: a map whose H rows are not whole tiles but 2H are (14x14) is tiled by image PAIRS — 7 tiles per pair instead of 8
            // (f8_chain.hip ChainCfg::STACKABLE); st.tiles then counts the tiles of a pair (chain_launch_groups: a device with fewer slots runs unstacked)
            a.stack = (net->opt.chain_stack && !st.cluster && chain_stackable(st.C, st.MID, st.H, st.W, st.cin0, tail)) ? 2 : 1;
            st.tiles = (a.stack * st.H + a.R - 1) / a.R;
            out_formats(a.q);
            st.inst = chain_fast(a, shortcut_blocks, nq > 0);
            chain_kernel_name(kb, sizeof kb, st.C, st.MID, st.H, st.W, st.cin0, tail, st.inst);
            st.args = a; break;
        }
        case S_BCHAIN: if (st.cluster) {
            const std::vector<int>& ch = nd.chain;
            BCChainArgs a{};
            a.nblk = (int)ch.size();
            for (int k = 0; k < a.nblk; ++k) {
                const Node& hk = ND[ch[k]];
                const Block& r = hk.blk;
                const Node& c2 = ND[r.b2];
                BChainBlk& B = a.blk[k];
                if (r.sc >= 0) {                                // the opening block's join: (body.2 << acc_shl) + (shortcut << res_shl)
                    B.wb = W8(c2.wf_off); B.bb = B32(c2.b_off);
                    B.r1 = fmt(c2);
                    B.relu1 = ND[hk.fused_add].relu;
                    a.tail = 1; a.wsc = W8(hk.wf_off); a.bsc = B32(hk.b_off);
                    B.relu_a = ND[T[c2.a].prod].cd.relu;        // (body.0's ReLU: mid0's format)
                    join_shifts(T[c2.out].fl - T[hk.out].fl, &B.acc_shl, &B.res_shl);
                    continue;
                }
                bind_basic_block(B, hk, ND[r.b0], c2);
                join_shifts(T[c2.out].fl - T[ND[r.b0].a].fl, &B.acc_shl, &B.res_shl);
            }
            a.pool = nd.pool >= 0 ? 1 : 0;
            const Tensor& x = T[ND[nd.fused_add].out];
            st.C = x.C; st.H = x.H; st.W = x.W;
            st.tiles = 8;                                       // the workgroups of one cluster
            out_formats(a.q);
            st.inst = bcchain_inst(a, nq > 0);                  // (requant_float = 1: the integer instance, as the 7x7 bottleneck chain)
            bcchain_kernel_name(kb, sizeof kb, st.inst);
            st.args = a; break;
        } else {
            const std::vector<int>& ch = nd.chain;
            BChainArgs a{};
            a.nblk = (int)ch.size();
            const bool ds = ND[ch[0]].blk.sc >= 0;
            for (int k = 0; k < a.nblk; ++k) {
                const Node& hk = ND[ch[k]];
                const Block& r = hk.blk;
                const bool hds = r.sc >= 0;                     // opening block: hk = its shortcut conv
                Node& c1 = ND[r.b0]; const Node& c2 = ND[r.b2];
                BChainBlk& B = a.blk[k];
                bind_basic_block(B, hk, c1, c2);
                if (k == 0) { a.acc_ok = 1; a.rq_int = rq_int; a.stream_ok = (hds || stream_bounded(net, c1.a)) ? 1 : 0; }   // identity first block: the stream it reads
                a.acc_ok = a.acc_ok && conv_acc_bounded(c1);
                a.stream_ok = a.stream_ok && stream_bounded(net, ND[hk.fused_add].out);
                // identity: (second conv << acc_shl) + (block input << res_shl); opening block: (second conv << acc_shl) + (shortcut << res_shl)
                join_shifts(T[c2.out].fl - (hds ? T[hk.out].fl : T[c1.a].fl), &B.acc_shl, &B.res_shl);
                if (hds) { a.wsc = W8(hk.wf_off); a.bsc = B32(hk.b_off); }
            }
            const Tensor& x = T[st.out.t];
            st.C = x.C; st.H = x.H; st.W = x.W;
            st.tiles = bchain_tiles_per_img(x.C, x.H, x.W);
            out_formats(a.q);
            st.inst = bchain_fast(a, ds, nq > 0);
            bchain_kernel_name(kb, sizeof kb, st.C, st.H, st.W, ds, st.inst);
            st.args = a; break;
        }
        case S_IR: {
            Node& na = ND[nd.blk.b0]; Node& nb = ND[nd.blk.b2];
            const Tensor& x = T[st.src_t];
            const Tensor& oT = T[nd.out];
            IRArgs a{};
            bind_ir_common(a, na, nb, x, oT);
            a.tiles_per_img = oT.H / a.R;
            a.acc_ok = conv_acc_bounded(na) && conv_acc_bounded(nb); a.rq_int = rq_int;
            fused_ir_kernel_name(kb, sizeof kb, x.Cs, nd.coutP, st.inst = fused_ir_inst(a, nd.coutP));
            st.args = a; break;
        }
        case S_IRK: {
            const Tensor& x = T[st.src_t];
            const Tensor& oT = T[nd.out];
            IRKArgs a{};
            bind_ir_common(a, ND[nd.blk.b0], ND[nd.blk.b2], x, oT);      // (wd4: pack_dwk_weights' dot4 image)
            a.K = ND[nd.blk.b2].cd.kernel; a.cin = x.Cs; a.cout = nd.coutP;
            a.tiles_per_img = (oT.H + a.R - 1) / a.R;
            a.QS = (oT.W + 3) / 4;
            a.dQS = fast_divisor((uint32_t)a.QS);
            a.dRQS = fast_divisor((uint32_t)(a.R * a.QS));
            irk_kernel_name(kb, sizeof kb, a.K, a.cout, st.inst = irk_inst(a));      // integer requantisation whatever requant_float says (as f8_dwk.hip)
            st.args = a; break;
        }
        case S_IRCHAIN: {
            const std::vector<int>& ch = nd.chain;
            const Tensor& x = T[st.src_t];
            IRChainArgs a{};
            a.nblk = (int)ch.size();
            a.acc_ok = 1; a.rq_int = rq_int;
            for (int k = 0; k < a.nblk; ++k) {
                const Block& r = ND[ch[k]].blk;
                const Node& c = ND[ch[k]]; Node& na = ND[r.b0]; Node& nb = ND[r.b2];
                IRChainBlk& B = a.blk[k];
                B.w0 = W8(na.w_off); B.b0 = B32(na.b_off);
                B.wd4 = W8(nb.rc_off); B.bd4 = B32(nb.cc_off);
                B.w4 = W8(c.w_off); B.b4 = B32(c.b_off);
                B.cin = T[na.a].Cs; B.cout = c.coutP; B.E32 = na.coutP;
                B.r1 = fmt(nb);
                B.r2 = fmt(c);
                B.relu_a = na.cd.relu; B.relu_b = nb.cd.relu; B.relu0 = c.cd.relu;
                if (c.fused_add >= 0) {                         // (project << acc_shl) + (block input << res_shl)
                    B.res = 1; B.relu1 = ND[c.fused_add].relu;
                    join_shifts(T[c.out].fl - T[na.a].fl, &B.acc_shl, &B.res_shl);
                }
                if (k + 1 < a.nblk) {
                    B.rq = fmt(ND[ND[ch[k + 1]].blk.b0]);
                    B.keep = ND[ch[k + 1]].fused_add >= 0;
                }
                a.acc_ok = a.acc_ok && conv_acc_bounded(na) && conv_acc_bounded(nb);
            }
            a.H = x.H; a.W = x.W;
            a.dW = fast_divisor((uint32_t)x.W);
            out_formats(a.q);
            st.inst = irchain_inst(a);
            irchain_kernel_name(kb, sizeof kb, st.inst);
            st.args = a; break;
        }
        case S_DWS: {
            Node& nb = ND[nd.blk.b0];
            const Tensor& oT = T[nd.out];
            DwsArgs a{};
            a.wd = W8(nb.w_off); a.bd = B32(nb.cc_off);           // the tap-major image; bias + 128 * sum(w) for unsigned inputs
            bind_dws_common(a, nb, T[st.src_t]);
            a.P = oT.H; a.Q = oT.W; a.R = nd.blk.R;
            dws_kernel_name(kb, sizeof kb, a, st.inst = dws_inst(a, nq));
            st.args = a; break;
        }
        case S_DWS7: {
            Node& nb = ND[nd.blk.b0];
            Dws7Args a{};
            a.wd4 = W8(nb.rc_off); a.bd4 = B32(nb.cc_off);        // the dot4 image; bias + 128 * sum(w) for unsigned inputs
            bind_dws_common(a, nb, T[st.src_t]);
            a.I = nd.blk.I7;
            a.pool = nd.pool >= 0 ? 1 : 0;
            dws7_kernel_name(kb, sizeof kb, a, st.inst = dws7_inst(a, nq));
            st.args = a; break;
        }
        case S_DW: {
            const Tensor& sT = T[st.src_t];
            const Tensor& oT = T[nd.out];
            DwArgs a{};
            a.w = W8(nd.w_off); a.bias = B32(nd.b_off);
            a.w4 = W8(nd.rc_off); a.bias4 = B32(nd.cc_off);
            const f8_conv_geom g = geom_of(nd);           // (a strip: one stride for both axes, the leading pad of each)
            a.H = sT.H; a.W = sT.W; a.P = oT.H; a.Q = oT.W; a.Cs = sT.Cs; a.stride = g.stride_h; a.pad = g.pad_top; a.pad_w = g.pad_left;
            a.in_signed = nd.cd.input_signed; a.relu0 = st.relu0; a.acc_ok = conv_acc_bounded(nd); a.rq_int = rq_int;
            a.k = g.kh; a.kw = g.kw; a.dil = nd.dil;
            out_formats(a.q);
            if (dw_general(nd)) {                                 // f8_dwk.hip: integer requantisation (requant1) whatever requant_float says
                st.inst = dwk_inst(a, out32, opt.dwk_dot4);
                dwk_kernel_name(kb, sizeof kb, a, st.inst);
            } else {
                st.inst = dwconv_inst(a, out32, nq, opt.dw_mma, opt.dw_dot4, net->max_batch);     // (the MMA kernel's index bound at the largest launch)
                dwconv_kernel_name(kb, sizeof kb, a, st.inst);
            }
            st.args = a; break;
        }
        case S_GCONV: {
            const Tensor& sT = T[st.src_t];
            const Tensor& oT = T[nd.out];
            GConvArgs a{};
            a.w = W8(nd.w_off); a.bias = B32(nd.b_off);
            a.ncc = nd.ncc;
            if (nd.ncc > 0) { a.rowcls = (const uint8_t*)W8(nd.rc_off); a.colcls = (const uint8_t*)W8(nd.cc_off); }
            a.H = sT.H; a.W = sT.W; a.P = oT.H; a.Q = oT.W; a.Cs = sT.Cs; a.stride = nd.cd.stride; a.pad = nd.cd.pad;
            gconv_tile(a.P, a.Q, a.stride, &a.R, &a.TW, &a.G);
            a.tiles_r = (a.P + a.R - 1) / a.R; a.tiles_c = (a.Q + a.TW - 1) / a.TW;
            a.PR = (a.R - 1) * a.stride + 3; a.PW = (a.TW - 1) * a.stride + 3;
            a.dIPP = fast_divisor((uint32_t)(a.PR * a.PW));
            a.dPW = fast_divisor((uint32_t)a.PW);
            a.dRTW = fast_divisor((uint32_t)(a.R * a.TW));
            a.dTW = fast_divisor((uint32_t)a.TW);
            a.relu0 = st.relu0;
            gconv_kernel_name(kb, sizeof kb, a);                  // integer requantisation whatever requant_float says (as f8_dwk.hip)
            out_formats(a.q); st.args = a; break;
        }
        case S_DECONV: {
            const Tensor& sT = T[st.src_t];
            const Tensor& oT = T[nd.out];
            DeconvArgs a{};
            a.w = W8(nd.w_off); a.w_bytes = (uint32_t)((size_t)nd.coutP * nd.ktot);
            a.bias = B32(nd.b_off);
            a.ncc = nd.ncc;
            if (nd.ncc > 0) { a.rowcls = (const uint8_t*)W8(nd.rc_off); a.colcls = (const uint8_t*)W8(nd.cc_off); }
            a.H = sT.H; a.W = sT.W; a.P = oT.H; a.Q = oT.W; a.CK = sT.Cs; a.coutP = nd.coutP; a.stride = nd.cd.stride; a.pad = nd.cd.pad;
            a.nph = a.stride * a.stride;
            for (int k = 0; k < a.nph; ++k) a.ph[k] = nd.dph[k];
            a.relu0 = st.relu0;
            snprintf(kb, sizeof kb, "%s", deconv_kernel_name(st.inst = deconv_inst(a)));      // integer requantisation whatever requant_float says (as f8_gconv.hip)
            out_formats(a.q); st.args = a; break;
        }
        case S_ADD: case S_REQUANT: {
            AddArgs a{};
            a.Cs = T[st.src_t].Cs; a.a_shl = st.acc_shl; a.b_shl = st.res_shl; a.relu = st.relu1;
            snprintf(kb, sizeof kb, "%s", add_kernel_name());
            out_formats(a.q); st.args = a; break;
        }
        case S_CONCAT: {
            const Tensor& oT = T[nd.out];
            ConcatArgs a{};
            a.K = (int)st.cat_t.size(); a.Cs = oT.Cs;
            int off = 0;
            for (int i = 0; i < a.K; ++i) {
                const Tensor& x = T[st.cat_t[i]];
                a.C[i] = x.C; a.Cs_src[i] = x.Cs; a.off[i] = off; a.shl[i] = oT.fl - x.fl;
                off += x.C;
            }
            snprintf(kb, sizeof kb, "%s", concat_kernel_name(st.inst = concat_inst(a, nd.bytes_mode)));
            out_formats(a.q); st.args = a; break;
        }
        case S_UPSAMPLE: {
            const Tensor& sT = T[st.cat_t[0]]; const Tensor& oT = T[nd.out];
            UpsampleArgs a{};
            a.C = oT.C; a.Cs = oT.Cs; a.Hs = sT.H; a.Ws = sT.W; a.P = oT.H; a.Q = oT.W; a.sh = nd.up_sh; a.sw = nd.up_sw;
            while (nd.up_mode == F8_UP_BILINEAR && (1 << a.k) < a.sh) ++a.k;
            a.dPQ = fast_divisor((uint32_t)(a.P * a.Q));
            a.dQ = fast_divisor((uint32_t)a.Q);
            a.dSh = fast_divisor((uint32_t)a.sh);
            a.dSw = fast_divisor((uint32_t)a.sw);
            a.dWs = fast_divisor((uint32_t)a.Ws);
            a.dVpp = fast_divisor((uint32_t)(a.Cs >> 4));
            snprintf(kb, sizeof kb, "%s", upsample_kernel_name(st.inst = upsample_inst(nd.up_mode == F8_UP_BILINEAR, nd.bytes_mode)));
            out_formats(a.q); st.args = a; break;
        }
        case S_CHANMAP: {
            const Tensor& oT = T[nd.out];
            ChanMapArgs a{};
            a.C = oT.C; a.Cs = oT.Cs; a.groups = nd.cm_groups; a.Cg = nd.cm_groups ? oT.C / nd.cm_groups : 0;
            a.K = nd.kind == N_SLICE ? 1 : nd.cm_groups;
            for (int i = 0; i < a.K; ++i) {                        // the table: the one source at offset first / i * Cg, or concat operand i at 0
                const bool fused = nd.cm_cat >= 0;
                a.Cs_src[i] = T[st.cat_t[fused ? i : 0]].Cs;
                a.off[i] = nd.kind == N_SLICE ? nd.cm_first : fused ? 0 : i * a.Cg;
            }
            a.dG = fast_divisor((uint32_t)std::max(a.groups, 1));
            snprintf(kb, sizeof kb, "%s", chanmap_kernel_name(st.inst = chanmap_inst(a, nd.bytes_mode)));
            out_formats(a.q); st.args = a; break;
        }
        case S_PIXMAP: {
            const Tensor& sT = T[st.cat_t[0]]; const Tensor& oT = T[nd.out];
            PixMapArgs a{};
            a.C = oT.C; a.Cs = oT.Cs; a.P = oT.H; a.Q = oT.W; a.Csrc = sT.C; a.Cs_src = sT.Cs; a.Hs = sT.H; a.Ws = sT.W;
            a.r = nd.pm_block; a.s2d = nd.kind == N_S2D; a.crd = nd.pm_order == F8_ORDER_CRD;
            a.dPQ = fast_divisor((uint32_t)(a.P * a.Q));
            a.dQ = fast_divisor((uint32_t)a.Q);
            a.dHsWs = fast_divisor((uint32_t)(a.Hs * a.Ws));
            a.dWs = fast_divisor((uint32_t)a.Ws);
            a.dR = fast_divisor((uint32_t)a.r);
            a.dRR = fast_divisor((uint32_t)(a.r * a.r));
            a.dC = fast_divisor((uint32_t)a.Csrc);
            snprintf(kb, sizeof kb, "%s", pixmap_kernel_name(st.inst = pixmap_inst(a, nd.bytes_mode)));
            out_formats(a.q); st.args = a; break;
        }
        case S_MUL: case S_HGATE: {
            const Tensor& oT = T[nd.out];
            MulArgs a{};
            a.C = oT.C; a.Cs = oT.Cs;
            if (st.kind == S_HGATE) {
                a.lim = 3 << oT.fl;
                st.inst = mul_inst(a, 0);
            } else {
                const Tensor& bT = T[nd.b];
                a.HW = oT.H * oT.W; a.dHW = fast_divisor((uint32_t)a.HW);
                a.bcast = bT.H * bT.W != a.HW; a.gate = nd.mul_gate >= 0; a.relu = st.relu1;
                if (a.gate) a.lim = 3 << bT.fl;
                a.ra = Requant::of(T[nd.a].fl - nd.md.a_fl, nd.md.a_signed != 0);
                a.rb = Requant::of(bT.fl - nd.md.b_fl, nd.md.b_signed != 0);
                if (nd.mul_table >= 0) {                             // b is looked up in the launch (f8_table.hip): the mul's record and the byte table
                    TableMulArgs ta{};
                    ta.bt = (const uint8_t*)W8(nd.tab_off);
                    st.inst = table_mul_inst(TableMulArgs{a, nullptr}, !out32);
                    a.dVpp = fast_divisor((uint32_t)(a.Cs / (st.inst == 1 ? 16 : 4)));
                    ta.m = a;
                    snprintf(kb, sizeof kb, "%s", table_mul_kernel_name(st.inst));
                    out_formats(ta.m.q); st.args = ta; break;
                }
                st.inst = mul_inst(a, out32 ? 1 : 2);
                a.dVpp = fast_divisor((uint32_t)(a.Cs / mul_vector_bytes(st.inst)));
            }
            snprintf(kb, sizeof kb, "%s", mul_kernel_name(st.inst));
            out_formats(a.q); st.args = a; break;
        }
        case S_TABLE: {
            const Tensor& oT = T[nd.out];
            TableArgs a{};
            a.C = oT.C; a.Cs = oT.Cs;
            const bool i8 = nd.bytes_mode && !out32;
            if (i8) {
                int slot_k[2];
                const int nr = table_slots(st.out, slot_k);      // (out_formats below sets q[k] from the same st.out.f8[k])
                for (int j = 0; j < nr; ++j) a.bt[slot_k[j]] = (const uint8_t*)W8(nd.tab_off + 256 * (size_t)j);
            } else a.t32 = B32(nd.tab_off);
            st.inst = table_inst(a, i8);
            a.dVpp = fast_divisor((uint32_t)(a.Cs / (st.inst == 1 ? 16 : 4)));
            snprintf(kb, sizeof kb, "%s", table_kernel_name(st.inst));
            out_formats(a.q); st.args = a; break;
        }
        case S_SUMPOOL: {
            const Tensor& sT = T[st.src_t]; const Tensor& oT = T[nd.out];
            SumPoolArgs a{};
            a.C = oT.C; a.Cs = oT.Cs; a.H = sT.H; a.W = sT.W; a.P = oT.H; a.Q = oT.W; a.k = nd.sum_k; a.stride = nd.sum_stride; a.pad = nd.sum_pad;
            a.lg = sumpool_wide_lg(a.k);
            a.dPQ = fast_divisor((uint32_t)(a.P * a.Q));
            a.dQ = fast_divisor((uint32_t)a.Q);
            a.dK = fast_divisor((uint32_t)a.k);
            a.dCg = fast_divisor((uint32_t)(a.Cs >> 2));
            snprintf(kb, sizeof kb, "%s", sumpool_kernel_name(st.inst = sumpool_inst(a.k, nd.sum_wide)));
            out_formats(a.q); st.args = a; break;
        }
        case S_MAXPOOL: {
            const Tensor& sT = T[st.src_t]; const Form& sF = sT.forms[st.src_f];
            const Tensor& oT = T[nd.out];
            PoolArgs a{};
            a.in_is_i8 = sF.kind == FORM_I8; a.in_signed = sF.sgn;
            a.H = sT.H; a.W = sT.W; a.P = oT.H; a.Q = oT.W; a.Cs = sT.Cs; a.k = nd.pk; a.stride = nd.pstride; a.pad = nd.ppad;
            snprintf(kb, sizeof kb, "%s", maxpool_kernel_name(st.inst = maxpool_inst(a)));
            out_formats(a.q); st.args = a; break;
        }
        case S_AVGPOOL: {
            const Tensor& sT = T[st.src_t];
            AvgArgs a{};
            a.HW = sT.H * sT.W; a.Cs = sT.Cs;
            snprintf(kb, sizeof kb, "%s", avgpool_kernel_name());
            out_formats(a.q); st.args = a; break;
        }
        case S_OUTPUT: {
            const Tensor& sT = T[st.src_t];
            OutArgs a{};
            a.C = sT.C; a.HW = sT.H * sT.W; a.Cs = sT.Cs; a.as_float = net->outs[st.out_k].as_float;
            st.inst = st.out_k >= 1 && opt.tap_tiled;      // output 0 stays on output_kernel (option tap_tiled, f8net.h)
            snprintf(kb, sizeof kb, "%s", st.inst ? tap_kernel_name(a.as_float) : output_kernel_name());
            st.args = a; break;
        }
        case S_ARGMAX: {
            const Tensor& sT = T[st.src_t]; const Tensor& oT = T[net->outs[st.out_k].t];
            const bool fused = nd.kind == N_UPSAMPLE && nd.argmax_k == st.out_k;      // st.node: the upsample inside the launch, else the marked tensor's producer
            ArgmaxArgs a{};
            a.C = oT.C; a.Cs = sT.Cs; a.Hs = sT.H; a.Ws = sT.W; a.P = oT.H; a.Q = oT.W;
            a.sh = fused ? nd.up_sh : 1; a.sw = fused ? nd.up_sw : 1;
            while (fused && nd.up_mode == F8_UP_BILINEAR && (1 << a.k) < a.sh) ++a.k;
            a.dSh = fast_divisor((uint32_t)a.sh);
            a.dSw = fast_divisor((uint32_t)a.sw);
            a.dQ4 = fast_divisor((uint32_t)((a.Q + 3) >> 2));
            a.dP = fast_divisor((uint32_t)a.P);
            snprintf(kb, sizeof kb, "%s", argmax_kernel_name(st.inst = argmax_inst(fused, fused && nd.up_mode == F8_UP_BILINEAR, net->outs[st.out_k].idx)));
            st.args = a; break;
        }
    }
    st.kernel = kb;
    return rc;
}

int f8_net_finalize(f8_net* net, int max_batch) {
    if (!net) return fail(F8_ERR_INVALID, "f8_net_finalize: null net");
    if (net->finalized) return fail(F8_ERR_STATE, "f8_net_finalize: already finalized");
    if (max_batch < 1) return fail(F8_ERR_INVALID, "f8_net_finalize: max_batch < 1");
    if (net->outs.empty()) return fail(F8_ERR_STATE, "f8_net_finalize: no output marked");
    if (net->nodes.empty() || net->nodes[0].kind != N_INPUT) return fail(F8_ERR_STATE, "f8_net_finalize: first node must be the input");
    plan_residual_joins(net);                       // 1:  a residual add rides in the epilogue of the later of its two producers
    plan_bottleneck_blocks(net, max_batch);         // 1b: bottleneck identity blocks (one launch, or body.0 + body.2 on the 7x7 maps)
    plan_dual_gemm_joins(net);                      // 1c: body.4 || shortcut of a stage-opening block as one dual GEMM
    plan_stage_opening_blocks(net);                 // 1d: whole stage-opening blocks (same resolution / stride 2)
    plan_stage_chains(net);                         // 1f: all consecutive bottleneck blocks of a stage in one launch
    plan_basic_block_chains(net);                   // 1g: the same for BasicBlocks
    plan_inverted_residuals(net);                   // 1e: MobileNet-V2 inverted residuals
    plan_inverted_residuals_k(net);                 // 1e3: inverted residuals around a depthwise 5x5 / 7x7 (option fuse_irk)
    plan_inverted_residual_chains(net);             // 1e2: runs of stride-1 inverted residuals in one launch (option fuse_irchain)
    plan_mobilenet_v2_head(net);                    // 1h: MobileNet-V2 head conv + depthwise + 1x1
    plan_last_conv_and_pool(net);                   // 1i: the last 1x1 conv + the average pool
    plan_depthwise_separable(net, max_batch);       // 1j: MobileNet-V1 depthwise-separable blocks in one launch (option fuse_dws)
    plan_depthwise_separable_7x7(net, max_batch);   // 1k: ... those on 7 x 7 output maps, and the average pool behind the last (option fuse_dws7)
    if (net->plan_bug >= 0) return fail(F8_ERR_STATE, "f8_net_finalize: planner bug: two fused launches claim conv node %d", net->plan_bug);
    plan_tensor_forms(net, max_batch);              // 2:  which forms of each tensor exist in HBM
    int rc = emit_steps(net, max_batch);            // 3:  the launches, packed weights, algorithmic bytes / ops
    if (rc) return rc;
    if ((rc = layout_arena(net, max_batch))) return rc;   // 4: lifetimes, first-fit arena
    net->max_batch = max_batch;
    for (Step& st : net->steps)                           // 5: the launch arguments the plan decides, the instances
        if ((rc = bind_step(net, st))) return rc;
    net->finalized = true;
    return F8_OK;
}

size_t f8_net_describe(const f8_net* net, char* buf, size_t cap) {
    std::string s;
    if (net && net->finalized) {
        char line[512];
        for (size_t i = 0; i < net->steps.size(); ++i) {
            const Step& st = net->steps[i];
            int n8 = (st.out.f8[0] >= 0) + (st.out.f8[1] >= 0);
            snprintf(line, sizeof line, "%3zu %-58s out[i32=%d i8=%d dense=%d] res=%d relu=%d/%d shl=%d/%d\n", i, st.name.c_str(),
                     st.out.f32 >= 0, n8, (int)st.dense, st.res_t >= 0, st.relu0, st.relu1, st.acc_shl, st.res_shl);
            s += line;
        }
        snprintf(line, sizeof line, "arena=%zu B (max_batch %d) weights=%zu B launches=%zu\n", net->arena_bytes, net->max_batch,
                 net->wblob.size(), net->steps.size());
        s += line;
    }
    if (buf && cap) { size_t n = std::min(cap - 1, s.size()); memcpy(buf, s.data(), n); buf[n] = 0; }
    return s.size() + 1;
}
int f8_net_num_launches(const f8_net* net) { return (net && net->finalized) ? (int)net->steps.size() : F8_ERR_STATE; }
size_t f8_net_arena_bytes(const f8_net* net) { return net ? net->arena_bytes : 0; }
size_t f8_net_weight_bytes(const f8_net* net) { return net ? net->wblob.size() : 0; }
int f8_net_output_fraclen(const f8_net* net) { return (net && !net->outs.empty()) ? (net->outs[0].idx ? 0 : net->tensors[net->outs[0].t].fl) : F8_ERR_STATE; }
size_t f8_net_output_elems(const f8_net* net) {
    if (!net || net->outs.empty()) return 0;
    const Tensor& t = net->tensors[net->outs[0].t];
    return (size_t)(net->outs[0].idx ? 1 : t.C) * t.H * t.W;
}

int f8_net_launch_info(const f8_net* net, int i, int N, char* name, size_t name_cap, double* alg_bytes, double* alg_ops) {
    if (!net || !net->finalized) return fail(F8_ERR_STATE, "f8_net_launch_info: not finalized");
    if (i < 0 || i >= (int)net->steps.size()) return fail(F8_ERR_INVALID, "f8_net_launch_info: index");
    const Step& st = net->steps[i];
    if (name && name_cap) { snprintf(name, name_cap, "%s", st.name.c_str()); }
    if (alg_bytes) *alg_bytes = st.bytes_per_img * N + st.bytes_const;
    if (alg_ops) *alg_ops = st.ops_per_img * N;
    return F8_OK;
}

int f8_net_launch_valu(const f8_net* net, int i, int N, double* essential_lane_ops) {
    if (!net || !net->finalized) return fail(F8_ERR_STATE, "f8_net_launch_valu: not finalized");
    if (i < 0 || i >= (int)net->steps.size() || !essential_lane_ops) return fail(F8_ERR_INVALID, "f8_net_launch_valu: index / null pointer");
    *essential_lane_ops = net->steps[i].valu_per_img * N;
    return F8_OK;
}

int f8_net_launch_kernel(const f8_net* net, int i, char* buf, size_t cap) {
    if (!net || !net->finalized) return fail(F8_ERR_STATE, "f8_net_launch_kernel: not finalized");
    if (i < 0 || i >= (int)net->steps.size()) return fail(F8_ERR_INVALID, "f8_net_launch_kernel: index");
    if (buf && cap) snprintf(buf, cap, "%s", net->steps[i].kernel.c_str());
    return F8_OK;
}

// Image groups resident at once in a chain launch (grid = groups x tiles per image, one workgroup per CU): a group walks
// ceil(N / groups) images, so of all group counts that need the same number of rounds the SMALLEST is taken — every group then
// has the same number of images (128 images on 18 groups of 14 tiles is 8 rounds for 2 groups and 7 for 16; on 16 groups it is 8
// for all, in the same time, on 224 CUs instead of 252) and the CUs left over run the other batches in flight.
// (taking every resident group instead — uneven rounds, the groups that finish early free their CUs — measured 1-3 % slower, round 4)
static int chain_groups(int N, int max_groups) {
    const int g = std::max(1, std::min(N, max_groups));
    const int rounds = (N + g - 1) / g;
    return (N + rounds - 1) / rounds;
}

// ------------------------------------------------------------------------------ executor
int f8_net_upload(f8_net* net) {
    if (!net || !net->finalized) return fail(F8_ERR_STATE, "f8_net_upload: not finalized");
    if (net->uploaded) return F8_OK;
    hipError_t e;
    const int parts_cap = std::max(net->opt.split, net->opt.arena_copies);     // arena copies: sub-batches of one run, or whole runs in flight (pipelining mode 2)
    if ((e = hipGetDevice(&net->device)) != hipSuccess) return hip_fail(e, "hipGetDevice");
    net->n_copies = parts_cap;
    { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, net->device) == hipSuccess && pr.multiProcessorCount > 0) net->num_cu = pr.multiProcessorCount; }
    net->arena_stride = round_up_z(std::max<size_t>(net->arena_bytes, 256), 4096);
    if ((e = hipMalloc((void**)&net->d_arena, net->arena_stride * parts_cap)) != hipSuccess) return hip_fail(e, "hipMalloc(arena)");
    if ((e = hipMalloc((void**)&net->d_w, std::max<size_t>(net->wblob.size(), 256))) != hipSuccess) return hip_fail(e, "hipMalloc(weights)");
    if (!net->wblob.empty() && (e = hipMemcpy(net->d_w, net->wblob.data(), net->wblob.size(), hipMemcpyHostToDevice)) != hipSuccess)
        return hip_fail(e, "hipMemcpy(weights)");
    if ((e = hipMalloc((void**)&net->d_err, 256)) != hipSuccess) return hip_fail(e, "hipMalloc(error words)");
    if ((e = hipMemset(net->d_err, 0, 256)) != hipSuccess) return hip_fail(e, "hipMemset(error words)");
    for (Step& st : net->steps) (void)bind_step(net, st);     // again, now with the weight pointers (the plan part cannot fail twice)
    for (const Step& st : net->steps)
        if ((st.kind == S_CHAIN || st.kind == S_BCHAIN) && !net->d_chain) {
            size_t xchg = kChainXchgBytes;
            for (const Step& c7 : net->steps)
                if (c7.kind == S_CHAIN) {
                    const Tensor& o7 = net->tensors[net->nodes[net->nodes[c7.node].fused_add].out];   // the stage's map (c7.out.t: the pooled tensor when the pool runs in the launch)
                    if (cchain_supported(o7.C, net->nodes[c7.node].cd.cin, o7.H, o7.W, o7.C, false)) xchg = std::max(xchg, cchain_xchg_bytes());   // (geometry; the last host is an identity block's body.4)
                } else if (c7.kind == S_BCHAIN && c7.cluster) xchg = std::max(xchg, bcchain_xchg_bytes());
            net->chain_stride = round_up_z(4096 + xchg, 4096);
            if ((e = hipMalloc((void**)&net->d_chain, net->chain_stride * parts_cap)) != hipSuccess) return hip_fail(e, "hipMalloc(chain scratch)");
            if ((e = hipMemset(net->d_chain, 0, net->chain_stride * parts_cap)) != hipSuccess) return hip_fail(e, "hipMemset(chain scratch)");
            // a host-visible mirror of the error word: a chain launch that gives up a halo wait stores its code there as well, and f8_net_run looks at it
            // (a host read: no synchronisation) before it issues anything — a caller that never calls f8_net_check still gets a status (VERDICT r4 #5d)
            if (hipHostMalloc((void**)&net->h_err, 64, hipHostMallocMapped) == hipSuccess) {
                *net->h_err = 0u;
                if (hipHostGetDevicePointer((void**)&net->h_err_dev, net->h_err, 0) != hipSuccess) { (void)hipHostFree(net->h_err); net->h_err = nullptr; net->h_err_dev = nullptr; }
            } else { net->h_err = nullptr; (void)hipGetLastError(); }
        }
    for (int p = 0; p < parts_cap; ++p)
        if (net->stem_zero_bytes && (e = hipMemset(net->d_arena + p * net->arena_stride + net->stem_zero_off, net->stem_zero_val, net->stem_zero_bytes)) != hipSuccess)
            return hip_fail(e, "hipMemset(stem halo)");
    if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "upload sync");
    net->uploaded = true;
    return F8_OK;
}

// Geometry of a chain launch (S_CHAIN / S_BCHAIN) over N images on num_cu compute units (0: 256 assumed).  *stack: ChainArgs::stack as bound
// (2 = tile columns of image pairs), set back to 1 where the slots do not hold a pair's tiles; *tiles: workgroups per tile column.  Returns the
// image groups (clusters, in the 7x7 cluster form) resident at once, 0 where the slots do not hold one column (one cluster): every workgroup
// of a chain launch must be resident.
static int chain_geometry(const Step& st, int N, int num_cu, int32_t* stack, int* tiles) {
    const int slots = (num_cu > 0 ? std::min(num_cu, 256) : 256) * st.wg_per_cu;
    *tiles = st.tiles;
    if (*stack == 2 && slots < st.tiles) {
        const int R = std::get<ChainArgs>(st.args).R;
        *stack = 1; *tiles = (st.H + R - 1) / R;
    }
    if (slots < *tiles) return 0;
    if (st.cluster) return cchain_clusters(N, slots);
    return chain_groups(*stack == 2 ? (N + 1) / 2 : N, slots / *tiles);
}

static int chain_launch_groups(const f8_net* net, const Step& st, int N, int32_t* stack) {
    int tiles = 0;
    const int ng = chain_geometry(st, N, net->num_cu, stack, &tiles);
    if (ng >= 1) return ng;
    if (st.cluster) fail(F8_ERR_STATE, "f8_net_run: the 7x7 stage-chain launch needs 8 co-resident workgroups, the device has %d compute units (plan with %s = 0)", net->num_cu,
                         st.kind == S_BCHAIN ? "fuse_bchain7" : "fuse_chain7");
    else fail(F8_ERR_STATE, "f8_net_run: a stage-chain launch needs %d co-resident workgroups per image, the device has %d compute units (plan with fuse_chain = 0 / fuse_bchain = 0)", tiles, net->num_cu);
    return 0;
}

int f8_net_launch_grid(const f8_net* net, int i, int N, int num_cu, int* tiles, int* groups, int* grid, int* stack) {
    if (!net || !net->finalized) return fail(F8_ERR_STATE, "f8_net_launch_grid: not finalized");
    if (i < 0 || i >= (int)net->steps.size() || N < 1 || !tiles || !groups || !grid || !stack) return fail(F8_ERR_INVALID, "f8_net_launch_grid: index / batch / null pointer");
    const Step& st = net->steps[i];
    *tiles = *groups = *grid = *stack = 0;
    if (st.kind != S_CHAIN && st.kind != S_BCHAIN) return F8_OK;
    int32_t sk = st.kind == S_CHAIN ? std::get<ChainArgs>(st.args).stack : 1;
    *groups = chain_geometry(st, N, num_cu, &sk, tiles);
    *stack = sk < 1 ? 1 : sk;
    *grid = *groups * (st.cluster ? 8 : *tiles);
    return F8_OK;
}

// What one run reads and writes: built on the stack by its entry point (begin_run) and read-only from there on; the handle keeps
// nothing of a call but the cross-run state (the run tag, the pipelining ring, the graph cache).
struct RunIO {
    enum Kind { I32, F32, U8, U8_NHWC } kind = I32;
    const void* in = nullptr;                  // the caller's images: NCHW planes of `kind`, U8_NHWC: pixels
    float scale = 0.f; int lo = 0, hi = 0;     // F32: rint(x * scale) clamped to [lo, hi]
    const int16_t* lut = nullptr;              // U8 / U8_NHWC: the 3 x 256 table on f8_net_run_u8's stack (launches copy it into their arguments)
    void* out = nullptr;                       // output 0
    void* bufs[F8_MAX_OUTPUTS - 1] = {}; bool have_bufs = false;   // outputs 1 .. (f8_net_set_output_buffers, consumed)
    hipEvent_t in_ready = nullptr;             // the producer of `in` (f8_net_set_input_ready, consumed)
};
// Does the launch of step st read the caller's buffer in this run?  The input step does, unless the stem launch reads it itself
// (raw_input) — which that launch cannot do for uint8 NHWC pixels: those go through the input step and the haloed form after all.
static bool reads_raw_input(const Step& st, const RunIO& io) {
    const bool stem_reads = st.raw_input && io.kind != RunIO::U8_NHWC;
    return st.kind == S_INPUT ? !stem_reads : stem_reads;
}
// The caller's buffer from element `off` on, as the launch's arguments describe it.  sgn: sign of the 8-bit format an int32 input is
// narrowed to without a requant (< 0: it is not) — values outside that format would wrap silently, so they are checked.
extern "C++" template <class A>
static void bind_raw_common(A& a, const f8_net* net, const RunIO& io, size_t off, int sgn) {
    if (io.kind == RunIO::F32) { a.xf = (const float*)io.in + off; a.scale = io.scale; a.qlo = io.lo; a.qhi = io.hi; }
    else if (io.kind != RunIO::I32) { a.xu8 = (const uint8_t*)io.in + off; memcpy(a.lut, io.lut, sizeof a.lut); }
    else if (net->opt.check_input_range && sgn >= 0) { a.err = net->d_err; const Requant f = Requant::of(0, sgn != 0); a.chk_lo = f.lo; a.chk_hi = f.hi; }
}
static void bind_raw_input(InArgs& a, const f8_net* net, const RunIO& io, size_t off, int sgn) {
    a.u8_nhwc = io.kind == RunIO::U8_NHWC; if (io.kind == RunIO::I32) a.x = (const int32_t*)io.in + off;
    bind_raw_common(a, net, io, off, sgn);
}
static void bind_raw_input(StemPoolArgs& a, const f8_net* net, const RunIO& io, size_t off, int sgn) {
    a.raw_kind = io.kind == RunIO::I32 ? 0 : io.kind == RunIO::F32 ? 1 : 2; if (io.kind == RunIO::I32) a.xi = (const int32_t*)io.in + off;
    bind_raw_common(a, net, io, off, sgn);
}

// Runs one launch for images [n0, n0 + N) of the batch; c0 = the chunk's first image inside the arena (for_each_launch).  Every
// sub-batch works in its OWN copy of the arena (index `part`): the arena packs tensors by lifetime assuming the steps of one batch
// run in order, so two sub-batches that are at different steps at the same time must not share it (a later, larger tensor of the
// sub-batch that is ahead would overlap an earlier tensor the other one is still reading).  The launch's arguments are st.args
// (bind_step) plus what this run decides: arena and caller pointers, the batch, the chain scratch.
static int run_step(const f8_net* net, const RunIO& io, const Step& st, int n0, int N, int c0, int part, hipStream_t s) {
    const auto& T = net->tensors;
    char* A = net->d_arena + (size_t)part * net->arena_stride;
    auto fp = [&](const Form& F) -> char* { return A + F.off + (size_t)c0 * F.bytes_per_img; };
    const Node& nd = net->nodes[st.node];
    auto fill_out = [&](int32_t** out32, QuantOut q[2]) {
        if (st.out.t < 0 || st.dense) return;
        const Tensor& o = T[st.out.t];
        if (st.out.f32 >= 0) *out32 = (int32_t*)fp(o.forms[st.out.f32]);
        for (int k = 0; k < 2; ++k) if (st.out.f8[k] >= 0) q[k].ptr = (int8_t*)fp(o.forms[st.out.f8[k]]);
    };
    // what a run adds to IRArgs, IRKArgs and IRChainArgs alike: the int8 block input, its int32 form where the (first) block joins, the output forms
    auto ir_io = [&](auto& a) {
        a.x8 = (const int8_t*)fp(T[st.src_t].forms[st.src_f]); a.N = N;
        if (st.res_t >= 0) a.xr = (const int32_t*)fp(T[st.res_t].forms[st.res_f]);
        fill_out(&a.out32, a.q);
    };
    // what a run adds to the arguments of a launch that reads one form of one tensor: the source, the batch, the output forms.  Returns the source's form.
    auto src_io = [&](auto& a, int32_t** out32) -> const Form& {
        const Form& sF = T[st.src_t].forms[st.src_f];
        a.x = (decltype(a.x))fp(sF); a.N = N;
        fill_out(out32, a.q);
        return sF;
    };
    // the source pointers of a gather step (Step::cat_t / cat_f): slot(k, i) = entry i of the launch's table for output form k, `entries` of them — source i,
    // or, where the step has a single source (upsample; a stand-alone slice / shuffle, whose table has one entry per group), that source for every entry
    auto gather_sources = [&](int entries, auto&& slot) {
        const bool one = st.cat_t.size() == 1;
        for (int k = 0; k < 2; ++k)
            if (!st.cat_f[k].empty())
                for (int i = 0; i < entries; ++i) { const size_t j = one ? 0 : (size_t)i; slot(k, i) = fp(T[st.cat_t[j]].forms[st.cat_f[k][j]]); }
    };
    char* const chain = net->d_chain ? net->d_chain + (size_t)part * net->chain_stride : nullptr;
    const uint32_t* chain_err = chain ? (const uint32_t*)chain + kChainErrWord : nullptr;
    auto chain_scratch = [&](ChainSync& cs) {
        if (!chain) return fail(F8_ERR_STATE, "f8_net_run: chain scratch missing");
        cs.sync = (uint32_t*)chain;
        cs.err = cs.sync + kChainErrWord; cs.err_host = net->h_err_dev; cs.epoch = net->epoch;
        cs.xchg = (int8_t*)(chain + 4096);
        cs.timeout_ticks = (uint32_t)std::min<long long>((long long)net->opt.chain_timeout_ms * 100000ll, 0x7fffffffll);
        return (int)F8_OK;
    };
    hipError_t e = hipSuccess;
    switch (st.kind) {
        case S_INPUT: {
            if (!reads_raw_input(st, io)) break;                               // the stem launch reads the caller's buffer
            const Tensor& o = T[st.out.t];
            InArgs a{}; a.N = N; a.C = o.C; a.H = o.H; a.W = o.W;
            int narrow = -1;                                                   // sign of the head format (an 8-bit form without a requant)
            for (auto& F : o.forms) {
                if (F.kind == FORM_I8) { if (F.n == 0) { a.out8 = (int8_t*)fp(F); a.Cs8 = o.Cs; a.xor8 |= Requant::of(0, F.sgn).bias_xor; narrow = F.sgn; } }
                else if (F.kind == FORM_I32) { a.out32 = (int32_t*)fp(F); a.Cs32 = o.Cs; }
                else { a.stem = (int8_t*)fp(F); a.Hp = F.Hp; a.Wp = F.Wp; a.pad = F.pad; a.xor8 |= Requant::of(0, F.sgn).bias_xor; narrow = F.sgn; }
            }
            bind_raw_input(a, net, io, (size_t)n0 * o.C * o.H * o.W, narrow);
            e = launch_input(a, st.inst, s);
            break;
        }
        case S_CONV: {
            const Form& sF = T[st.src_t].forms[st.src_f];
            ConvArgs a = std::get<ConvArgs>(st.args);
            a.x = (const int8_t*)fp(sF); a.x_bytes = (uint32_t)(sF.bytes_per_img * N); a.M = N * a.PQ;
            if (st.res_t >= 0) a.res = (const int32_t*)fp(T[st.res_t].forms[st.res_f]);
            if (st.src2_t >= 0) { const Form& F2 = T[st.src2_t].forms[st.src2_f]; a.x2 = (const int8_t*)fp(F2); a.x2_bytes = (uint32_t)(F2.bytes_per_img * N); }
            fill_out(&a.out32, a.q);
            const int C = T[nd.out].C;
            switch (st.variant) {
                case V_FC: e = launch_fc_dense(a, (char*)io.out + (size_t)n0 * C * 4, C, net->outs[0].as_float, chain_err, net->epoch, s); break;
                case V_POOL: e = launch_conv1x1_pool(a, s); break;
                case V_S2WREG: e = launch_conv3x3s2_wreg(a, s); break;
                case V_WSTAT: e = launch_conv1x1_wstat(a, st.inst, net->num_cu, net->opt.wstat_grid_div, s); break;
                case V_WREG: e = launch_conv1x1_wreg(a, s); break;
                case V_PATCH3X3: e = launch_conv3x3_patch(a, nd.cd.cin, s); break;
                default: e = launch_conv(a, nd.tile, st.inst, s);      // V_IGEMM
            }
            break;
        }
        case S_HEAD2: case S_STEMPOOL: {
            const Tensor& sT = T[st.src_t]; const Form& sF = sT.forms[st.src_f];
            StemPoolArgs a = std::get<StemPoolArgs>(st.args);
            a.x = (const int8_t*)fp(sF); a.x_bytes = (uint32_t)(sF.bytes_per_img * N); a.N = N;
            if (st.kind == S_STEMPOOL) a.wpc = net->opt.stem_wpc;
            a.grid_div = net->opt.stem_grid_div;
            if (reads_raw_input(st, io)) {                               // the raw network input, read by this launch (the input step launches nothing)
                a.rC = sT.C; a.rH = sT.H; a.rW = sT.W; a.xor8 = Requant::of(0, sF.sgn).bias_xor;
                bind_raw_input(a, net, io, (size_t)n0 * sT.C * sT.H * sT.W, sF.sgn ? 1 : 0);
            }
            fill_out(&a.out32, a.q);
            e = launch_stem_pool(a, st.inst, s);
            break;
        }
        case S_FUSED: case S_P12: {
            const Form& xF = T[st.src_t].forms[st.src_f];
            FusedArgs a = std::get<FusedArgs>(st.args);
            a.x8 = (const int8_t*)fp(xF); a.x_bytes = (uint32_t)(xF.bytes_per_img * N); a.N = N;
            if (st.res_t >= 0) a.xr = (const int32_t*)fp(T[st.res_t].forms[st.res_f]);     // identity block: its int32 input
            fill_out(&a.out32, a.q);
            e = st.variant == V_OPENER ? launch_fused_opener(a, st.inst, s) : st.variant == V_P12 ? launch_fused_p12(a, s) : launch_fused_bottleneck(a, s);
            break;
        }
        case S_CHAIN: {
            ChainArgs a = std::get<ChainArgs>(st.args);
            const Form& xF = T[st.src_t].forms[st.src_f];
            if (xF.kind == FORM_I8) a.x8in = (const int8_t*)fp(xF); else a.xr = (const int32_t*)fp(xF);     // (an identity first block reads the int32 stream)
            if (a.tail) a.m2in = (const int8_t*)fp(T[st.src2_t].forms[st.src2_f]);
            a.N = N;
            if ((a.NG = chain_launch_groups(net, st, N, &a.stack)) < 1) return F8_ERR_STATE;
            fill_out(&a.out32, a.q);
            if (const int rc = chain_scratch(a.cs)) return rc;
            e = launch_chain(a, st.inst, st.C, st.MID, st.H, st.W, st.cin0, s);
            break;
        }
        case S_BCHAIN: if (st.cluster) {
            BCChainArgs a = std::get<BCChainArgs>(st.args);
            const Tensor& xs = T[st.src_t];
            if (st.res_t >= 0) { a.m0in = (const int8_t*)fp(xs.forms[st.src_f]); a.x8sc = (const int8_t*)fp(T[st.res_t].forms[st.res_f]); }   // the opening block's join
            else a.xr = (const int32_t*)fp(xs.forms[st.src_f]);
            a.N = N;
            { int32_t one = 1; if ((a.NG = chain_launch_groups(net, st, N, &one)) < 1) return F8_ERR_STATE; }
            fill_out(&a.out32, a.q);
            if (const int rc = chain_scratch(a.cs)) return rc;
            e = launch_bcchain(a, st.inst, s);
            break;
        } else {
            BChainArgs a = std::get<BChainArgs>(st.args);
            const Tensor& xs = T[st.src_t];
            if (st.res_t >= 0) { a.x8in = (const int8_t*)fp(xs.forms[st.src_f]); a.x8sc = (const int8_t*)fp(xs.forms[st.res_f]); }     // opening block: two int8 forms
            else a.xr = (const int32_t*)fp(xs.forms[st.src_f]);
            a.N = N;
            { int32_t one = 1; if ((a.NG = chain_launch_groups(net, st, N, &one)) < 1) return F8_ERR_STATE; }
            fill_out(&a.out32, a.q);
            if (const int rc = chain_scratch(a.cs)) return rc;
            e = launch_bchain(a, st.inst, st.C, st.H, st.W, s);
            break;
        }
        case S_IR: { IRArgs a = std::get<IRArgs>(st.args); ir_io(a); e = launch_fused_ir(a, T[st.src_t].Cs, nd.coutP, st.inst, s); break; }
        case S_IRK: { IRKArgs a = std::get<IRKArgs>(st.args); ir_io(a); e = launch_fused_irk(a, st.inst, s); break; }
        case S_IRCHAIN: { IRChainArgs a = std::get<IRChainArgs>(st.args); ir_io(a); e = launch_irchain(a, st.inst, s); break; }
        case S_DWS: { DwsArgs a = std::get<DwsArgs>(st.args); int32_t* none = nullptr; src_io(a, &none); e = launch_dws(a, st.inst, s); break; }
        case S_DWS7: { Dws7Args a = std::get<Dws7Args>(st.args); src_io(a, &a.out32); e = launch_dws7(a, st.inst, net->num_cu, s); break; }
        case S_DW: {
            DwArgs a = std::get<DwArgs>(st.args); src_io(a, &a.out32);
            e = (a.k == 3 && a.kw == 3 && a.pad == 1 && a.dil == 1) ? launch_dwconv(a, st.inst, s) : launch_dwk(a, st.inst, s);      // (general depthwise: f8_dwk.hip)
            break;
        }
        case S_GCONV: { GConvArgs a = std::get<GConvArgs>(st.args); a.x_bytes = (uint32_t)(src_io(a, &a.out32).bytes_per_img * N); e = launch_gconv(a, s); break; }
        case S_DECONV: { DeconvArgs a = std::get<DeconvArgs>(st.args); a.x_bytes = (uint32_t)(src_io(a, &a.out32).bytes_per_img * N); e = launch_deconv(a, st.inst, s); break; }
        case S_SUMPOOL: { SumPoolArgs a = std::get<SumPoolArgs>(st.args); src_io(a, &a.out32); e = launch_sumpool(a, st.inst, s); break; }
        case S_MAXPOOL: { PoolArgs a = std::get<PoolArgs>(st.args); src_io(a, &a.out32); e = launch_maxpool(a, st.inst, s); break; }
        case S_AVGPOOL: { AvgArgs a = std::get<AvgArgs>(st.args); src_io(a, &a.out32); e = launch_avgpool(a, s); break; }
        case S_ADD: case S_REQUANT: {
            const Tensor& sT = T[st.src_t];
            AddArgs a = std::get<AddArgs>(st.args);
            a.a = (const int32_t*)fp(sT.forms[st.src_f]);
            if (st.kind == S_ADD) a.b = (const int32_t*)fp(T[st.res_t].forms[st.res_f]);
            a.M = N * sT.H * sT.W;
            fill_out(&a.out32, a.q);
            e = launch_add(a, s);
            break;
        }
        case S_CONCAT: {
            ConcatArgs a = std::get<ConcatArgs>(st.args);
            gather_sources(a.K, [&](int k, int i) -> const void*& { return a.src[k][i]; });
            a.M = N * T[st.out.t].H * T[st.out.t].W;
            fill_out(&a.out32, a.q);
            e = launch_concat(a, st.inst, s);
            break;
        }
        case S_UPSAMPLE: {
            UpsampleArgs a = std::get<UpsampleArgs>(st.args);
            gather_sources(1, [&](int k, int) -> const void*& { return a.src[k]; });
            a.N = N;
            fill_out(&a.out32, a.q);
            e = launch_upsample(a, st.inst, s);
            break;
        }
        case S_CHANMAP: {
            ChanMapArgs a = std::get<ChanMapArgs>(st.args);
            gather_sources(a.K, [&](int k, int i) -> const void*& { return a.src[k][i]; });
            a.M = N * T[st.out.t].H * T[st.out.t].W;
            fill_out(&a.out32, a.q);
            e = launch_chanmap(a, st.inst, s);
            break;
        }
        case S_PIXMAP: {
            PixMapArgs a = std::get<PixMapArgs>(st.args);
            gather_sources(1, [&](int k, int) -> const void*& { return a.src[k]; });
            a.N = N;
            fill_out(&a.out32, a.q);
            e = launch_pixmap(a, st.inst, s);
            break;
        }
        case S_TABLE: {
            TableArgs a = std::get<TableArgs>(st.args);
            const Tensor& o = T[st.out.t];
            a.src = (const int8_t*)fp(T[st.src_t].forms[st.src_f]);
            a.M = N * o.H * o.W;
            fill_out(&a.out32, a.q);
            e = launch_table(a, st.inst, s);
            break;
        }
        case S_MUL: case S_HGATE: {
            if (std::holds_alternative<TableMulArgs>(st.args)) {
                TableMulArgs a = std::get<TableMulArgs>(st.args);
                const Tensor& o = T[st.out.t];
                a.m.a = (const int8_t*)fp(T[st.src_t].forms[st.src_f]); a.m.b = fp(T[st.res_t].forms[st.res_f]);
                a.m.M = N * o.H * o.W;
                fill_out(&a.m.out32, a.m.q);
                e = launch_table_mul(a, st.inst, s);
                break;
            }
            MulArgs a = std::get<MulArgs>(st.args);
            const Tensor& o = T[st.out.t];
            if (st.kind == S_MUL) { a.a = (const int8_t*)fp(T[st.src_t].forms[st.src_f]); a.b = fp(T[st.res_t].forms[st.res_f]); }
            else a.b = fp(T[st.src_t].forms[st.src_f]);
            a.M = N * o.H * o.W;
            fill_out(&a.out32, a.q);
            e = launch_mul(a, st.inst, s);
            break;
        }
        case S_OUTPUT: {
            OutArgs a = std::get<OutArgs>(st.args);
            a.x = (const int32_t*)fp(T[st.src_t].forms[st.src_f]); a.N = N;
            char* const buf = st.out_k ? (char*)io.bufs[st.out_k - 1] : (char*)io.out;
            a.out = buf + (size_t)n0 * a.C * a.HW * 4; a.err = chain_err; a.epoch = net->epoch;
            e = st.inst ? launch_tap(a, s) : launch_output(a, s);
            break;
        }
        case S_ARGMAX: {
            ArgmaxArgs a = std::get<ArgmaxArgs>(st.args);
            a.x = (const int32_t*)fp(T[st.src_t].forms[st.src_f]); a.N = N;
            char* const buf = st.out_k ? (char*)io.bufs[st.out_k - 1] : (char*)io.out;
            a.out = buf + (size_t)n0 * a.P * a.Q * net->outs[st.out_k].idx;      // the sub-batch's first image: elements of index_bytes, not of 4
            a.err = chain_err; a.epoch = net->epoch;
            e = launch_argmax(a, st.inst, s);
            break;
        }
    }
    if (e != hipSuccess) return hip_fail(e, st.name.c_str());
    return F8_OK;
}

// Cuts the batch into up to F8_SPLIT (default 2, max 4) equal sub-batches (the last takes the remainder), never more than arena
// copies or images.  Returns the number of parts and their starts in cut[0..parts].
static int split_batch(const f8_net* net, int N, int cut[5]) {
    const int want = std::min(net->opt.split, net->n_copies > 0 ? net->n_copies : net->opt.split);
    const int parts = std::min(want, N);
    cut[0] = 0; cut[1] = N;
    if (parts < 2) return 1;
    for (int p = 0; p < parts; ++p) cut[p] = p * (N / parts);
    cut[parts] = N;
    return parts;
}
// The parts of one run: split_batch, except that pipelining mode 2 runs every batch unsplit (it overlaps whole runs instead).
static int run_parts(const f8_net* net, int N, int cut[5]) {
    const int parts = split_batch(net, N, cut);     // (cut[0] = 0)
    if (net->pipelined == 2) cut[1] = N;
    return net->pipelined == 2 ? 1 : parts;
}

// Measured tile choice: every implicit-GEMM conv step is timed on the device with each tile that has a kernel
// instance (HIP events, best of a few repetitions, on garbage activations: integer kernels are data-independent in
// time) and keeps the fastest.  Results are bit-identical for every tile; only the plan description changes.
int f8_net_autotune(f8_net* net, int N, void* stream) {
    if (!net || !net->finalized) return fail(F8_ERR_STATE, "f8_net_autotune: not finalized");
    if (N < 1 || N > net->max_batch) return fail(F8_ERR_INVALID, "f8_net_autotune: N=%d outside [1,%d]", N, net->max_batch);
    int rc = f8_net_upload(net);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    int cut[5];
    (void)split_batch(net, N, cut);
    const int n_launch = cut[1] - cut[0];                      // images of one sub-batch launch
    const RunIO io{};                                          // (a conv step reads and writes the arena only)
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return fail(F8_ERR_HIP, "f8_net_autotune: events");
    int changed = 0;
    for (auto& st : net->steps) {
        if (st.variant != V_IGEMM) continue;                       // (conv_igemm_kernel steps only)
        Node& nd = net->nodes[st.node];
        const ConvTile keep = nd.tile;
        ConvTile best = keep; float best_ms = 1e30f;
        for (int c = 0; c < 4; ++c) {
            ConvTile t = keep; t.bm = kIgemmCandBm[c]; t.bn = kIgemmCandBn[c];
            if (!igemm_tile_admissible(nd, t)) continue;
            nd.tile = t;
            (void)bind_step(net, st);                                  // the instance follows the tile (ring depth)
            if (run_step(net, io, st, 0, n_launch, 0, 0, s) != F8_OK) { (void)hipGetLastError(); continue; }   // no instance
            float ms_min = 1e30f;
            for (int rep = 0; rep < 3; ++rep) {
                (void)hipEventRecord(e0, s);
                for (int k = 0; k < 4; ++k) (void)run_step(net, io, st, 0, n_launch, 0, 0, s);
                (void)hipEventRecord(e1, s);
                if (hipEventSynchronize(e1) != hipSuccess) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); return fail(F8_ERR_HIP, "f8_net_autotune: sync"); }
                float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
                if (ms < ms_min) ms_min = ms;
            }
            const float bias = (t.bm == keep.bm && t.bn == keep.bn) ? 0.97f : 1.0f;   // switch only for a clear (> 3 %) win
            if (ms_min * bias < best_ms) { best_ms = ms_min * bias; best = t; }
        }
        nd.tile = best;
        (void)bind_step(net, st);
        if (best.bm != keep.bm || best.bn != keep.bn) { ++changed; label_conv_step(net, st, nd); }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return changed;
}

// Chunked execution.  The fused bottleneck blocks of a stage run in chunks of images, block after block per chunk: a chunk's
// int32 stream (78 MB for 24 images at 56x56, 103 MB for 64 images at 28x28) is still in the memory-side cache when the next
// block reads it.  Measured, 56x56 identity blocks alone: 3.12 us per image in one 128-image launch, 2.66 us in 32-image
// launches.  Whole net at bs 128, same box: 56x56 chunks of 16 / 24 / 32 / 40 / 48 images = +1.0 / +2.1 / +1.4 / -1.4 / -0.7 %;
// then 28x28 chunks of 32 / 48 / 64 / 80 / 96 = +1.7 / +2.5 / +2.9 / +2.8 / +1.1 %; the 14x14 tensors (103 MB per batch) need
// none.  Applies in every schedule (a sub-batch of 64 images still runs its 56x56 blocks in chunks: non-pipelined run
// 73.4k -> 75.1k img/s).
// Defaults are DERIVED from two numbers, not hand-fitted per net:
//   cache : the int32 stream of a chunk (bytes per image of the wider of the block's int32-sized input and output maps: 3.2 MB
//           at 56x56x256, 1.6 MB at 28x28x512, 0.8 MB at 14x14x1024) should fit Options::chunk_budget_mb (96 MiB = 3/8 of the
//           256 MiB memory-side cache);
//   fill  : a chunk launch must still fill the chip: >= 85 % of (CUs x resident workgroups per CU) workgroups.
// chunk = max(cache, fill): 56x56 -> 30 images (cache), 28x28 -> 64 (fill: 7 tiles per image, 2 workgroups per CU),
// 14x14 -> 128 (fill: 2 tiles per image, 1 per CU), which is what sweeps over explicit sizes had found (24-32 / 64 / 128).
// chunk56 / chunk28 / chunk14 override (0 = whole batch).  Every chunk offset must keep the I32T blocks of the group's tensors
// aligned (chunk * H*W a multiple of 32 pixels, for the source map AND a stage-opening block's half-resolution output):
// chunks are multiples of 2 / 8 / 32 images.
static int chunk_gran(int W) { return W == 56 ? 2 : (W == 28 ? 8 : 32); }
static int step_chunk(const f8_net* net, int i) {        // nominal images per chunk of step i (0 = not chunked)
    const Step& st = net->steps[i];
    if (st.kind != S_FUSED) return 0;                    // (chunking the stage-opening convs as well: -3 %, more launches than locality)
    const Node& nd = net->nodes[st.node];
    const Block& r = nd.blk;
    const bool opener = st.variant == V_OPENER;
    const Options& o = net->opt;
    if (r.sc >= 0 && !(opener ? o.chunk_opener : o.chunk_ds)) return 0;
    const Tensor& x = net->tensors[st.src_t];
    if (x.W != x.H || !(x.W == 56 || x.W == 28 || x.W == 14)) return 0;
    int chunk = x.W == 56 ? o.chunk56 : (x.W == 28 ? o.chunk28 : o.chunk14);
    const int gran = chunk_gran(x.W);
    if (chunk < 0) {
        size_t per_img = (size_t)x.H * x.W * x.Cs * 4;
        if (st.out.t >= 0) { const Tensor& y = net->tensors[st.out.t]; per_img = std::max(per_img, (size_t)y.H * y.W * y.Cs * 4); }
        const int cache = (int)std::min<size_t>(((size_t)o.chunk_budget_mb << 20) / std::max<size_t>(per_img, 1), 1 << 20) / gran * gran;
        const int mid = net->nodes[r.b0].cd.cout;
        const int tiles = std::max(1, (opener ? x.H / 2 : x.H) / std::max(1, r.R));        // workgroups per image
        const int slots = (net->num_cu > 0 ? net->num_cu : 256) * ((opener || mid > 128) ? 1 : 2);
        const int fill = ((slots * 85 / 100 + tiles - 1) / tiles + gran - 1) / gran * gran;
        chunk = std::max(cache, fill);
    }
    chunk = chunk / gran * gran;
    return chunk;
}
// f(step index, first image of the chunk, images) for every kernel launch of a run over N images, in launch order.
// A group = consecutive chunkable steps at one resolution with the same nominal chunk; the batch is cut into equal chunks
// (no tiny tail), and not at all when it exceeds the nominal chunk by less than a quarter.
extern "C++" template <class F>
static int for_each_launch(const f8_net* net, int N, F&& f) {
    const int ns = (int)net->steps.size();
    for (int i = 0; i < ns;) {
        const int nominal = step_chunk(net, i);
        const int W = nominal > 0 ? net->tensors[net->steps[i].src_t].W : 0;
        int k = nominal > 0 ? (N + nominal - 1) / nominal : 1;
        if (nominal > 0 && (long)N * 4 <= (long)nominal * 5) k = 1;
        if (k > 1) {
            const int gran = chunk_gran(W);
            const int chunk = ((N + k - 1) / k + gran - 1) / gran * gran;
            int j = i;
            while (j < ns && step_chunk(net, j) == nominal && net->tensors[net->steps[j].src_t].W == W) ++j;
            for (int c0 = 0; c0 < N; c0 += chunk)
                for (int kk = i; kk < j; ++kk) { const int rc = f(kk, c0, std::min(chunk, N - c0)); if (rc) return rc; }
            i = j;
        } else {
            const int rc = f(i, 0, N);
            if (rc) return rc;
            ++i;
        }
    }
    return F8_OK;
}
// all launches of one run for images [n0, n0 + N) of the network input, on stream s, in arena copy `part`
static int run_steps(const f8_net* net, const RunIO& io, int n0, int N, int part, hipStream_t s) {
    return for_each_launch(net, N, [&](int k, int c0, int cn) { return run_step(net, io, net->steps[k], n0, cn, c0, part, s); });
}

// ---- the schedules of a run (run_common picks exactly one) ----

// The internal streams and the fork / join events.  The streams are ONE set per device, shared by every handle of the process.
// HIP maps streams onto a few hardware queues (GPU_MAX_HW_QUEUES, default 4) in creation order: the first handle's streams got a
// queue each, a later handle's shared queues with them and its concurrent sub-batches / batches in flight serialised — measured,
// ResNet-18 with three batches in flight: the handle created first 330 k img/s, every later one 308 k (all 332 k with
// GPU_MAX_HW_QUEUES=16; tools/prof_intmodel.py).  Work of two handles on one stream is ordered, which costs nothing they would not
// contend for anyway.  (hipGraph capture needs streams of its own: a capture must not see another handle's launches.)
static int ensure_aux(f8_net* net) {
    if (net->aux[0] && !(net->opt.graph && net->aux_shared)) return F8_OK;
    if (net->aux[0]) {                               // `graph` was switched on after the pooled streams were taken: streams of its own
        for (int k = 0; k < 4; ++k) { (void)hipStreamSynchronize(net->aux[k]); net->aux[k] = nullptr; }
        net->aux_shared = false;
    }
    static std::mutex pool_mu;
    static hipStream_t pool[64][4] = {};
    const int dv = net->device;
    if (net->opt.shared_streams && !net->opt.graph && dv >= 0 && dv < 64) {
        std::lock_guard<std::mutex> lk(pool_mu);
        for (int k = 0; k < 4; ++k) {
            if (pool[dv][k]) continue;
            hipError_t e = hipStreamCreateWithFlags(&pool[dv][k], hipStreamNonBlocking);
            if (e != hipSuccess) { pool[dv][k] = nullptr; return hip_fail(e, "hipStreamCreate"); }
        }
        for (int k = 0; k < 4; ++k) net->aux[k] = pool[dv][k];
        net->aux_shared = true;
    } else
    for (int k = 0; k < 4; ++k) {
        hipError_t e = hipStreamCreateWithFlags(&net->aux[k], hipStreamNonBlocking);
        if (e != hipSuccess) return hip_fail(e, "hipStreamCreate");
    }
    for (int k = 0; k < 5; ++k) {
        if (net->aux_ev[k]) continue;
        hipError_t e = hipEventCreateWithFlags(&net->aux_ev[k], hipEventDisableTiming);
        if (e != hipSuccess) return hip_fail(e, "hipEventCreate");
    }
    return F8_OK;
}
// Lagged fork of a pipelined run: the n internal streams order themselves behind earlier runs on their arena copy by stream order;
// towards the caller they only wait for the state of `s` at the entry of the run `lag` entries back (header contract) — fewer while
// the ring is still filling or after the caller changed streams — and for this run's input, which that dependency does not cover.
static void lagged_fork(f8_net* net, hipStream_t s, int lag, const hipStream_t* streams, int n, hipEvent_t in_ready) {
    if (!net->start_ev[0]) for (int k = 0; k < 4; ++k) (void)hipEventCreateWithFlags(&net->start_ev[k], hipEventDisableTiming);
    if (net->prev_stream != s) net->pipe_count = 0;
    const int cur = net->start_idx;
    (void)hipEventRecord(net->start_ev[cur], s);
    hipEvent_t dep = net->start_ev[(cur - std::min(net->pipe_count, lag) + 4) & 3];
    for (int k = 0; k < n; ++k) { (void)hipStreamWaitEvent(streams[k], dep, 0); if (in_ready) (void)hipStreamWaitEvent(streams[k], in_ready, 0); }
    net->start_idx = (cur + 1) & 3; ++net->pipe_count; net->prev_stream = s;
}
// Profiled: the parts back to back on the caller's stream, one event after every launch; a step's time is the sum over its launches (parts x chunks).
static int run_profiled_pass(f8_net* net, const RunIO& io, int parts, const int cut[5], hipStream_t s, float* ms, int cap) {
    const int ns = (int)net->steps.size();
    if (cap < ns) return fail(F8_ERR_INVALID, "f8_net_run_profiled: ms capacity %d < %d launches", cap, ns);
    std::vector<int> owner;                          // step index of every launch, in order
    for (int p = 0; p < parts; ++p) {
        owner.push_back(-1);                         // start marker of the part
        (void)for_each_launch(net, cut[p + 1] - cut[p], [&](int k, int, int) { owner.push_back(k); return 0; });
    }
    const int ne = (int)owner.size();
    if (net->n_events < ne) {
        if (net->events) { for (int i = 0; i < net->n_events; ++i) (void)hipEventDestroy(net->events[i]); delete[] net->events; }
        net->events = new hipEvent_t[ne]; net->n_events = ne;
        for (int i = 0; i < ne; ++i) { hipError_t e = hipEventCreate(&net->events[i]); if (e != hipSuccess) return hip_fail(e, "hipEventCreate"); }
    }
    int pos = 0;
    for (int p = 0; p < parts; ++p) {
        (void)hipEventRecord(net->events[pos++], s);
        const int rc = for_each_launch(net, cut[p + 1] - cut[p], [&](int k, int c0, int cn) {
            const int r = run_step(net, io, net->steps[k], cut[p], cn, c0, p, s);
            (void)hipEventRecord(net->events[pos++], s);
            return r;
        });
        if (rc) return rc;
    }
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "f8_net_run_profiled: sync");
    for (int i = 0; i < ns; ++i) ms[i] = 0.f;
    for (int q = 1; q < ne; ++q) {
        if (owner[q] < 0) continue;
        float t = 0.f;
        (void)hipEventElapsedTime(&t, net->events[q - 1], net->events[q]);
        ms[owner[q]] += t;
    }
    // an input step that launched nothing (the stem launch read the caller's buffer) has no duration: the two events around it are ~5 us apart on their own
    for (int i = 0; i < ns; ++i)
        if (net->steps[i].kind == S_INPUT && !reads_raw_input(net->steps[i], io)) ms[i] = 0.f;
    return F8_OK;
}
// Alternating whole batches (pipelining mode 2): run i executes UNSPLIT on internal stream / arena copy i % D, so that consecutive
// runs are in flight together — the same occupancy as concurrent sub-batches, but every launch covers the whole batch (twice the
// workgroups per launch: at 128 images the latency-bound launches of the late stages fill the chip).  Options::pipeline_depth D
// (2..4, at most the arena copies) runs are in flight: the fork lags D-1 entries (and, by stream order, run i-D on the same arena
// copy); join: `s` waits for this run.
static int run_alternating(f8_net* net, const RunIO& io, int N, hipStream_t s) {
    if (const int rc = ensure_aux(net)) return rc;
    const int D = std::max(2, std::min(net->opt.pipeline_depth, net->n_copies));
    const int slot = net->alt_idx % D;
    lagged_fork(net, s, D - 1, &net->aux[slot], 1, io.in_ready);
    net->alt_idx = (slot + 1) % D;
    if (const int rc = run_steps(net, io, 0, N, slot, net->aux[slot])) return rc;
    (void)hipEventRecord(net->aux_ev[1 + slot], net->aux[slot]);
    (void)hipStreamWaitEvent(s, net->aux_ev[1 + slot], 0);
    return F8_OK;
}
// The parts one after the other on the caller's stream: a run of one part, and F8_SPLIT_STREAMS=0 (rocprofv3 runs: the same
// launches, their durations not inflated by the overlap of the sub-batches).
static int run_serial(const f8_net* net, const RunIO& io, int parts, const int cut[5], hipStream_t s) {
    for (int p = 0; p < parts; ++p)
        if (const int rc = run_steps(net, io, cut[p], cut[p + 1] - cut[p], p, s)) return rc;
    return F8_OK;
}
// Independent sub-batches on the internal streams: while one is in a layer's tail / epilogue phase the others keep the CUs busy.
// Fork from and join to `s` with events (no host sync); lagged: the fork of a pipelined run (lagged_fork).
static int run_forked(f8_net* net, const RunIO& io, int parts, const int cut[5], hipStream_t s, bool lagged) {
    if (lagged) lagged_fork(net, s, 1, net->aux, parts, io.in_ready);
    else {
        (void)hipEventRecord(net->aux_ev[0], s);
        for (int k = 0; k < parts; ++k) (void)hipStreamWaitEvent(net->aux[k], net->aux_ev[0], 0);
        net->pipe_count = 0;
    }
    // optional stagger: sub-batch p starts only after sub-batch p-1 has finished its first `lag` launches, so that the
    // streams do not march through the memory-bound and the latency-bound layers in lock step
    const int lag = net->opt.stagger >= 0 ? net->opt.stagger : (net->pipelined ? net->opt.stagger_pipelined : 2);   // measured: lag 0/1/2/4/8 = 56.06/56.37/56.65/56.34/55.1 k img/s
    // the launches of every part (chunked where a part is larger than a chunk), submitted round-robin so that no stream's
    // queue starts late
    struct Launch { int k, c0, cn; };
    std::vector<Launch> plan[4];
    size_t longest = 0;
    for (int p = 0; p < parts; ++p) {
        (void)for_each_launch(net, cut[p + 1] - cut[p], [&](int k, int c0, int cn) { plan[p].push_back({k, c0, cn}); return 0; });
        longest = std::max(longest, plan[p].size());
    }
    for (size_t t = 0; t < longest; ++t)
        for (int p = 0; p < parts; ++p) {
            if (t >= plan[p].size()) continue;
            const Launch& L = plan[p][t];
            if (const int rc = run_step(net, io, net->steps[L.k], cut[p], L.cn, L.c0, p, net->aux[p])) return rc;
            if (lag > 0 && (int)t == lag - 1 && p + 1 < parts) {
                if (!net->lag_ev[p]) (void)hipEventCreateWithFlags(&net->lag_ev[p], hipEventDisableTiming);
                (void)hipEventRecord(net->lag_ev[p], net->aux[p]);
                (void)hipStreamWaitEvent(net->aux[p + 1], net->lag_ev[p], 0);
            }
        }
    for (int k = 0; k < parts; ++k) { (void)hipEventRecord(net->aux_ev[1 + k], net->aux[k]); (void)hipStreamWaitEvent(s, net->aux_ev[1 + k], 0); }
    return F8_OK;
}
// F8_GRAPH=1 around run_forked: the second call with the same (input, output, N, stream) captures its launches into a hipGraph (the
// internal streams join the capture through the fork event, which is why a captured run forks unlagged); later calls replay it with
// one hipGraphLaunch.  The legacy null stream cannot be captured: the graph then lives on an internal stream fenced by events.
static int graph_replay(const f8_net* net, hipStream_t user_s) {
    hipStream_t gs = user_s ? user_s : net->aux[3];
    if (gs != user_s) { (void)hipEventRecord(net->aux_ev[0], user_s); (void)hipStreamWaitEvent(gs, net->aux_ev[0], 0); }
    hipError_t e = hipGraphLaunch(net->g_exec, gs);
    if (e != hipSuccess) return hip_fail(e, "hipGraphLaunch");
    if (gs != user_s) { (void)hipEventRecord(net->aux_ev[4], gs); (void)hipStreamWaitEvent(user_s, net->aux_ev[4], 0); }
    return F8_OK;
}
static int run_graphed(f8_net* net, const RunIO& io, int N, int parts, const int cut[5], hipStream_t user_s) {
    const bool same = net->g_in == io.in && net->g_out == io.out && net->g_N == N && net->g_stream == user_s;
    if (same && net->g_exec) return graph_replay(net, user_s);
    if (!same) {
        if (net->g_exec) { (void)hipGraphExecDestroy(net->g_exec); net->g_exec = nullptr; }
        net->g_in = io.in; net->g_out = io.out; net->g_N = N; net->g_stream = user_s; net->g_warm = 0;
    }
    if (net->g_warm++ < 1) return run_forked(net, io, parts, cut, user_s, net->pipelined != 0);   // a new key's first call runs eagerly (one-time kernel attribute calls happen there)
    hipStream_t gs = user_s ? user_s : net->aux[3];
    hipError_t e = hipStreamBeginCapture(gs, hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) return hip_fail(e, "hipStreamBeginCapture");
    const int rc = run_forked(net, io, parts, cut, gs, false);
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(gs, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) return hip_fail(e, "hipStreamEndCapture");
    e = hipGraphInstantiate(&net->g_exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) { net->g_exec = nullptr; return hip_fail(e, "hipGraphInstantiate"); }
    return graph_replay(net, user_s);
}
// What every run does first, whatever its schedule: the checks, the upload, the run's tag, the wait for the input's producer.
static int run_prologue(f8_net* net, const RunIO& io, int N, hipStream_t s) {
    if (!net || !net->finalized) return fail(F8_ERR_STATE, "f8_net_run: not finalized");
    if (net->outs.size() > 1 && !io.have_bufs)
        return fail(F8_ERR_STATE, "f8_net_run: this net has %d outputs: hand over the buffers of outputs 1 .. with f8_net_set_output_buffers before every run", (int)net->outs.size());
    if (N < 1 || N > net->max_batch) return fail(F8_ERR_INVALID, "f8_net_run: N=%d outside [1,%d]", N, net->max_batch);
    if (!io.in || !io.out) return fail(F8_ERR_INVALID, "f8_net_run: null pointer");
    if (const int rc = f8_net_upload(net)) return rc;
    if (net->opt.check_device) {       // the arena, the weights and the internal streams belong to the device of the upload
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess || dev != net->device)
            return fail(F8_ERR_STATE, "f8_net_run: current device %d, but this net lives on device %d (hipSetDevice before the call; one handle per device)", dev, net->device);
    }
    // this run's tag for the chain error words: a word an EARLIER run left behind (a transient halo time-out nobody collected with
    // f8_net_check) neither cuts this run's waits short nor poisons its logits; it stays where it is for f8_net_check to report.
    // (A replayed hipGraph carries the tag of its capture: there the word is sticky until f8_net_check, as it was before round 5.)
    if (net->h_err) {
        const uint32_t hw = *(volatile uint32_t*)net->h_err;
        if (hw) return fail(F8_ERR_HIP, "f8_net_run: a stage-chain launch of an earlier run gave up waiting for a neighbouring tile (code 0x%x of run tag %u): the logits of that run are "
                                        "poisoned (NaN / INT32_MIN); call f8_net_check to collect the error and re-arm the handle", hw & 0xffu, hw >> 8);
    }
    net->epoch = net->epoch % 0xffffffu + 1u;
    if (io.in_ready) (void)hipStreamWaitEvent(s, io.in_ready, 0);   // the producer of this run's input; every schedule forks from / runs on `s`
    return F8_OK;
}

static int run_common(f8_net* net, const RunIO& io, int N, void* stream, float* ms, int cap) {
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = run_prologue(net, io, N, s)) return rc;
    int cut[5];
    const int parts = run_parts(net, N, cut);
    if (ms) return run_profiled_pass(net, io, parts, cut, s, ms, cap);
    const bool streams = net->opt.split_streams != 0;
    if (net->pipelined == 2 && net->n_copies >= 2 && streams) return run_alternating(net, io, N, s);
    if (parts == 1 || !streams) return run_serial(net, io, parts, cut, s);
    if (const int rc = ensure_aux(net)) return rc;
    // (the replay key knows one int32 input and one output buffer: other runs issue plain launches)
    if (net->opt.graph && parts <= 3 && io.kind == RunIO::I32 && net->outs.size() == 1) return run_graphed(net, io, N, parts, cut, s);
    return run_forked(net, io, parts, cut, s, net->pipelined != 0);
}

int f8_net_num_parts(const f8_net* net, int N) {
    if (!net || !net->finalized) return fail(F8_ERR_STATE, "f8_net_num_parts: not finalized");
    int cut[5]; return run_parts(net, N, cut);
}

int f8_net_step_launches(const f8_net* net, int i, int N) {
    if (!net || !net->finalized) return fail(F8_ERR_STATE, "f8_net_step_launches: not finalized");
    if (i < 0 || i >= (int)net->steps.size()) return fail(F8_ERR_INVALID, "f8_net_step_launches: launch index out of range");
    int cut[5];
    const int parts = run_parts(net, N, cut);
    int n = 0;
    for (int p = 0; p < parts; ++p)
        (void)for_each_launch(net, cut[p + 1] - cut[p], [&](int k, int, int) { n += (k == i); return 0; });
    return n;
}

// ---- the run entries.  Each consumes the two one-shots (begin_run) before any check of its own: a call that fails for whatever
// reason leaves nothing armed for a later, unrelated run (by then the caller's event or buffers may be gone) ----
static RunIO begin_run(f8_net* net, const void* in, void* out) {
    RunIO io; io.in = in; io.out = out;
    if (!net) return io;
    io.in_ready = net->input_ready; net->input_ready = nullptr;
    io.have_bufs = net->out_bufs_set; net->out_bufs_set = false;
    if (io.have_bufs) memcpy(io.bufs, net->out_bufs, sizeof io.bufs);
    return io;
}
// sign of the network input's consumers (0 unsigned, 1 signed, < 0 status)
static int input_sign(const f8_net* net, const char* who) {
    const Tensor& in = net->tensors[net->nodes[0].out];
    int sgn = -1;
    for (int c : in.consumers) {
        const Node& nd = net->nodes[c];
        if (nd.kind != N_CONV && nd.kind != N_LINEAR && nd.kind != N_DECONV) return fail(F8_ERR_UNSUPPORTED, "%s: the input must feed convolutions", who);
        if (sgn >= 0 && sgn != (nd.cd.input_signed ? 1 : 0)) return fail(F8_ERR_UNSUPPORTED, "%s: consumers disagree on signedness", who);
        sgn = nd.cd.input_signed ? 1 : 0;
    }
    if (sgn < 0) return fail(F8_ERR_UNSUPPORTED, "%s: the input has no consumer", who);
    return sgn;
}
// the head format an image entry can quantise to: any 8-bit fraclen with `normalize`, the pixel values themselves (unsigned, fraclen 8) without
static int check_input_format(const f8_net* net, int normalize, int sgn, const char* who) {
    const int fl = net->tensors[net->nodes[0].out].fl;
    if (normalize && (fl < 0 || fl > (sgn ? 7 : 8))) return fail(F8_ERR_INVALID, "%s: input fraclen %d outside [0,%d]", who, fl, sgn ? 7 : 8);
    if (!normalize && (fl != 8 || sgn))
        return fail(F8_ERR_INVALID, "%s: normalize == 0 needs an unsigned input at fraclen 8 (fix_train.py:689-692), net has fl %d %s", who, fl, sgn ? "signed" : "unsigned");
    return F8_OK;
}

int f8_net_run(f8_net* net, const int32_t* input, void* output, int N, void* stream) {
    return run_common(net, begin_run(net, input, output), N, stream, nullptr, 0);
}
int f8_net_run_profiled(f8_net* net, const int32_t* input, void* output, int N, void* stream, float* ms, int cap) {
    const RunIO io = begin_run(net, input, output);
    if (!ms) return fail(F8_ERR_INVALID, "f8_net_run_profiled: null ms");
    return run_common(net, io, N, stream, ms, cap);
}
int f8_net_run_f32(f8_net* net, const float* images, int normalize, void* output, int N, void* stream) {
    RunIO io = begin_run(net, images, output);
    if (!net || !net->finalized) return fail(F8_ERR_STATE, "f8_net_run_f32: not finalized");
    if (!images) return fail(F8_ERR_INVALID, "f8_net_run_f32: null pointer");
    const int sgn = input_sign(net, "f8_net_run_f32");
    if (sgn < 0) return sgn;
    if (const int rc = check_input_format(net, normalize, sgn, "f8_net_run_f32")) return rc;
    io.kind = RunIO::F32;              // (normalize == 0: images are in [0,1], asserted >= 0 by the reference; 8-bit storage)
    io.scale = normalize ? (float)(1 << net->tensors[net->nodes[0].out].fl) : 255.f; io.lo = sgn ? -127 : 0; io.hi = sgn ? 127 : 255;
    return run_common(net, io, N, stream, nullptr, 0);
}
int f8_net_run_u8(f8_net* net, const uint8_t* images, int nhwc, int normalize, const float* mean, const float* stdv, void* output, int N, void* stream) {
    RunIO io = begin_run(net, images, output);
    if (!net || !net->finalized) return fail(F8_ERR_STATE, "f8_net_run_u8: not finalized");
    if (!images) return fail(F8_ERR_INVALID, "f8_net_run_u8: null pointer");
    const Tensor& in = net->tensors[net->nodes[0].out];
    if (in.C > 3 && normalize) return fail(F8_ERR_UNSUPPORTED, "f8_net_run_u8: mean / std are given for 3 channels");
    const int sgn = input_sign(net, "f8_net_run_u8");
    if (sgn < 0) return sgn;
    if (normalize && (!mean || !stdv)) return fail(F8_ERR_INVALID, "f8_net_run_u8: normalize needs mean and std");
    if (const int rc = check_input_format(net, normalize, sgn, "f8_net_run_u8")) return rc;
    for (int c = 0; normalize && c < 3; ++c) if (!(stdv[c] != 0.f)) return fail(F8_ERR_INVALID, "f8_net_run_u8: std[%d] is zero", c);
    // The decoder-side pipeline of the reference, per pixel value k of channel c, in the float32 operations torch executes
    // (fix_train.py:299-329 transforms.ToTensor / Normalize, then :683-692):
    //   t = float(k) / 255                        ToTensor
    //   normalize == 0:  x_int = round_half_even(255 * t)                  (== k; fraclen 8)
    //   normalize != 0:  t = (t - mean[c]) / std[c];  x_int = clamp(round_half_even(t * 2^fl), +-127 or [0,255])   (fix_quant)
    // A uint8 has 256 values: the whole pipeline is a 3 x 256 table built here on the host (IEEE single precision, one
    // rounding per operation as in torch) and looked up inside the input kernel.
    int16_t lut[3 * 256];
    const float scale = (float)(1 << (normalize ? in.fl : 0));
    const float lo = sgn ? -127.f : 0.f, hi = sgn ? 127.f : 255.f;
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 256; ++k) {
            volatile float t = (float)k / 255.0f;              // volatile: one rounding per operation, no contraction / excess precision
            int v;
            if (!normalize) { volatile float r = 255.0f * t; v = (int)__builtin_rintf(r); }
            else {
                volatile float d = t - mean[c];
                volatile float q = d / stdv[c];
                volatile float r = q * scale;
                float rr = __builtin_rintf(r);
                rr = rr < lo ? lo : (rr > hi ? hi : rr);
                v = (int)rr;
            }
            lut[c * 256 + k] = (int16_t)v;
        }
    io.kind = nhwc ? RunIO::U8_NHWC : RunIO::U8; io.lut = lut;
    return run_common(net, io, N, stream, nullptr, 0);
}

}  // extern "C"
