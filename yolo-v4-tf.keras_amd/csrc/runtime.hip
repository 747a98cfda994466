// runtime.hip -- host side of libyolo4hip: the C ABI of include/yolo4hip.h, the 110-conv plan
// (reference custom_layers.py:100-198 cspdarknet53 + yolov4_neck), the buffer plan and the executor.
//
// Plan notes
//  * conv index == call order below == Keras creation order == Darknet blob order (reference utils.py:19-21).
//  * every Concatenate of the reference is realised as ONE NHWC buffer whose channel slices are written in
//    place by the producing convs; UpSampling2D is the 2x2-replicating store of the
//    producing 1x1 conv; each residual Add is the epilogue of its 3x3 conv.
//  * activations for max_batch images are carved out of the caller's workspace once, at bind time.
#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "conv_tiles.h"
#include "kernels.h"

namespace y4 {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

struct View {
    int buf = -1;          // buffer id
    int h = 0, w = 0, cstride = 0, coff = 0, c = 0;     // rows (over the input's H) and columns (over W)
};
struct Buffer {
    int h, w, channels;
    bool f32;              // raw heads are float32 whatever the compute dtype
    size_t offset = 0;     // byte offset in the act workspace (for max_batch images)
    size_t bytes = 0;
};
enum OpKind { OP_STEM, OP_CONV, OP_SPP };
struct Op {
    OpKind kind;
    int conv = -1;
    View in, out, res;
    bool has_res = false, upsample = false, out_f32 = false;
    int conv2 = -1;        // fused CSP pair: second conv index (main-in), its output view and the channel split
    View out2;
    int split = 0;
    char name[16];
};
struct Layer {
    y4_layer_desc d;       // (in_side / out_side: -1 on a non-square handle)
    int in_h, in_w, out_h, out_w;
    int cout_pad;
    int fused_with = -1;   // >= 0: this layer's rows live in layer `fused_with`'s packed matrix at row `fused_row`
    int fused_row = 0;
    int extra_rows = 0;    // rows appended by a fused partner
    size_t w_off, scale_off, shift_off;   // byte offsets in the wts workspace
    bool has_tail = false;                // a chain can run this 1x1 conv as a tail: its weights are also kept in
    size_t tail_off = 0;                  // fragment order (pack_tail_weights) at this offset
    bool has_frag = false;                // a 3x3 stride-1 conv the halo2 tiles can run (16-bit, cin % 64 == 0): its weights are also kept
    size_t frag_off = 0;                  // in MFMA-fragment order (pack_conv_frag32) at this offset
};

// A run of ops executed as one kernel (conv_chain.h): head = 3x3 conv with residual Add and 64 output channels,
// then one or two 1x1 convs; the second reads Concatenate([first tail's output, route]).
struct Chain {
    int head, tail[2];      // op indices (tail[1] = -1 for a 2-conv chain)
    bool store_x;           // the head's output has other consumers and is still written (y4_ctx::stores_x adds retention)
    bool lds_pair = false;  // the tail runs from the head's tile kept in LDS (128/256 channels), not from registers
    // "Alternative" run (conv_chain.h CFG 4): the 64 -> 64 tail of run `alt_of` as a HEAD chained straight to that run's conv
    // over the concat (tail[0] here).  In force only while run `alt_of` cannot exist because its own head executes inside
    // a residual-block kernel.
    int alt_of = -1;
};

// A residual block "1x1 conv -> 3x3 conv + Add(block input)" executed as one spatially tiled kernel (resblock.hip)
struct ResRun {
    int head, tail;         // op indices of the 1x1 and the 3x3 conv
    int c;                  // channels (64 | 128): the tuner decides per channel group
    size_t blob_off = 0;    // fragment-ordered weights + affine in the wts workspace
};

// Every scheduling choice of a handle: which kernel runs each op.  The plan (Op, Chain, ResRun) is fixed once y4_create_hw
// returns; the setters and the autotuner write only this, and y4_copy_schedule copies it whole.
struct Schedule {
    struct Run {
        bool enabled = true;          // y4_autotune turns a run off when its separate kernels measure faster
        int tile = 0;                 // the head's tile when it runs chained (0 = heuristic); tile[head] stays the unfused choice
    };
    std::vector<int> tile;            // per op: 0 = heuristic
    std::vector<Run> run;             // per Chain
    bool fuse_stem = false;           // convs 0+1 as one kernel (stem_down.hip): op 0 launches it into op 1's output view, op 1 is a no-op
    bool fuse_chains = false;         // the runs as one kernel each
    // the stage kernel and the residual-block kernels (group 0 = C 128, 1 = C 64): `_on` = requested, `_enabled` = the tuner's verdict
    bool stage_on = false, stage_enabled = true;
    bool res_on = false, res_enabled[2] = {true, true};
    // sub-batching: ops [0, sub_last_op] run over `sub_images` images at a time (keeps the large early
    // activations of one sub-batch resident in the 256 MiB Infinity Cache between producer and consumer)
    int sub_images = 0, sub_last_op = -1;
    // y4_autotune may pick halo2 tile ids (conv_halo2_kernel.h: v_mfma_32x32x16, another fp32 summation order than the 16x16x32 tiles)
    bool allow_halo2 = false;
};
// Would two handles run the same kernels for the same tiles (y4_autotune_pair)?  The switches and sub-batching, not the tiles
// and verdicts the tuner writes.  A new switch goes into the struct and, if a pair must agree on it, here.
static bool same_switches(const Schedule& a, const Schedule& b) {
    return a.fuse_stem == b.fuse_stem && a.fuse_chains == b.fuse_chains && a.stage_on == b.stage_on && a.res_on == b.res_on &&
           a.sub_images == b.sub_images && a.sub_last_op == b.sub_last_op;
}

// One entry of y4_set_tiles / y4_get_tiles.  A plain conv's entry is its tile id.  The head of a run carries two choices in one
// entry, so that a get -> set round trip loses neither: -(run tile + 1000 * stand-alone tile) while the run executes as one
// kernel (0: with the heuristic tile; plain -t leaves the stand-alone tile as it is), its stand-alone tile (> 0) while it runs
// as separate kernels.  Either tile may be a split-K id, base + 100 e (conv_tiles.h).
struct TileEntry { int run, own; bool chained; };      // chained: entry <= 0
static TileEntry decode_entry(int v) { return v < 0 ? TileEntry{(-v) % 1000, (-v) / 1000, true} : TileEntry{0, v, v == 0}; }
static int encode_entry(int run, int own) { return -(run + 1000 * own); }

// A score-decay mode of the NMS stage as the handle keeps it (y4_set_nms_soft, y4_set_nms_matrix)
struct DecayMode {
    int method = 0;              // 0: off
    float sigma = 0.5f;
    float min_score = -1.0f;     // < 0: the config's score_threshold
    int top_k = 4096;
};

}  // namespace y4

using namespace y4;

struct y4_ctx {
    y4_config cfg;
    int es;                           // element size of the compute dtype
    int H, W;                         // input rows / columns (multiples of 32)
    int hcs;                          // padded channels of a raw head
    int nbox;
    int64_t flops_per_image = 0;
    int64_t weight_floats = 0;
    std::vector<Layer> layers;
    std::vector<Buffer> bufs;
    std::vector<Op> ops;
    View heads[3];
    std::vector<Chain> chains;        // 3x3+Add -> 1x1 (-> 1x1 over the concat) runs found in the plan
    // the first CSP stage (convs 2..7) as one spatially tiled kernel (csp_stage.hip): ops [stage_first, stage_last];
    // stage_first < 0 when the plan / dtype does not allow it
    int stage_first = -1, stage_last = -1;
    size_t stage_blob_off = 0;
    std::vector<ResRun> resruns;      // residual blocks of the 128- and 64-channel stages as one kernel each
    // ---- the plan above is fixed once y4_create_hw returns; this is what the setters and the tuner change
    Schedule sched;
    // a tuner permission and tuner scratch, not choices: y4_copy_schedule does not carry them
    bool allow_splitk = false;        // y4_autotune may pick split-K tile ids (conv_tiles.h); their counters + partial sums live at splitk_off
    int force_chain = -1;             // the tuner times this alternative run while the residual-block kernels are switched off
    bool stage_active() const { return stage_first >= 0 && sched.stage_on && sched.stage_enabled; }
    const ResRun* res_of(int oi, bool* is_head) const {
        if (!sched.res_on) return nullptr;
        for (const ResRun& r : resruns)
            if ((r.head == oi || r.tail == oi) && sched.res_enabled[r.c == 128 ? 0 : 1]) { if (is_head) *is_head = r.head == oi; return &r; }
        return nullptr;
    }
    bool heads_res(int oi) const { bool is_head = false; return res_of(oi, &is_head) && is_head; }
    // does this run execute as one kernel under the current settings?
    bool chain_active(const Chain& ch) const {
        const int ci = (int)(&ch - chains.data());
        if (!sched.fuse_chains || !sched.run[ci].enabled) return false;
        if (ch.alt_of >= 0) return ci == force_chain || res_of(chains[ch.alt_of].head, nullptr) != nullptr;
        if (force_chain >= 0 && chains[force_chain].alt_of == ci) return false;
        return res_of(ch.head, nullptr) == nullptr;
    }
    // workspace layout
    size_t act_bytes = 0, wts_bytes = 0;
    size_t zero_off = 0, dbox_off = 0, keys_off = 0, counts_off = 0, status_off = 0, scratch_off = 0, splitk_off = 0, obj_off = 0;
    // the cells' objectness logits beside the raw heads (kernels.h: ConvObjDesc): head i's are those of its images [0, obj_n[i])
    // -- written by the head conv's own launch, so they ARE the stored logits; y4_set_heads writes heads only and voids them
    int obj_n[3] = {-1, -1, -1};
    int cells_per_img = 0, cell_base[3] = {0, 0, 0};
    // decode's per-image candidate counters are zero (nms_kernel resets them); false: the next decode clears them itself
    bool counts_clean = false;
    int counts_n = 0;
    uint32_t cand_cap = 0;
    char* act = nullptr;
    char* wts = nullptr;
    bool weights_ready = false;
    // timing session (y4_timing_begin/end): per-op HIP events recorded by y4_predict
    std::vector<hipEvent_t> t_events;
    int t_max_steps = 0, t_steps = 0, t_per_step = 0, t_n = 0;
    std::vector<int> t_slot_op;       // op index credited with each event interval of a step
    std::vector<char> t_rec;          // per launch: record an event after it?
    bool t_coarse = false;            // events only where the op kind changes (stem | conv run | spp | conv run | decode | nms)
    bool t_recorded_this_call = false;
    // images of the current call are uint8 frames at network size (y4_forward_u8 / y4_predict_u8): the stem divides by 255
    bool img_u8 = false;
    // activation buffers share memory when their lifetimes do not overlap (y4_set_workspace_aliasing): a quarter of the
    // workspace, a hotter working set for the Infinity Cache; intermediate tensors are then not retained after a forward
    bool alias_bufs = false;
    // y4_set_retain_head_inputs: the outputs of convs 92 / 100 / 108 -- the head convs' inputs -- are written to HBM (also where an
    // LDS pair would keep them on chip) and live to the end of the forward: y4_head_grad reads them
    bool retain_head_in = false;
    // level 2 of the same switch: the inputs of convs 92 / 100 / 108 (the outputs of convs 91 / 99 / 107) live to the end of the
    // forward too: y4_block_grad reads them
    bool retain_block_in = false;
    // y4_set_box_loss: the box term y4_loss and the gradient entry points evaluate (kernels.h: BOX_GIOU / BOX_CIOU).  Host-only,
    // no workspace effect, and no scheduling choice: y4_copy_schedule does not carry it
    int box_kind = BOX_GIOU;
    // y4_set_nms_rule: the pair rule of the NMS kernel, read at every y4_decode_nms / y4_decode_nms_mapped / y4_predict* call.
    // Host-only like box_kind: no workspace effect, not carried by y4_copy_schedule, not in a checkpoint
    int nms_kind = 0;
    float nms_beta = 1.0f;
    int nms_agnostic = 0;
    // y4_set_nms_soft / y4_set_nms_matrix: score decay instead of hard suppression in nms_over (soft_nms.hip, matrix_nms.hip).
    // Host-only, as the rule.  At most one of the two is on; one that is off keeps its parameters
    DecayMode soft, matrix;
    // is the head's output of this run written to HBM?  (an LDS pair in front of a head conv: also when that conv's input is retained)
    bool stores_x(const Chain& ch) const { return ch.store_x || (ch.lds_pair && retain_head_in && ops[ch.tail[0]].out_f32); }
};

namespace {

struct Builder {
    y4_ctx& c;
    explicit Builder(y4_ctx& ctx) : c(ctx) {}

    View alloc(int h, int w, int ch, bool f32 = false) {
        Buffer b{h, w, ch, f32};
        c.bufs.push_back(b);
        View v;
        v.buf = (int)c.bufs.size() - 1; v.h = h; v.w = w; v.cstride = ch; v.coff = 0; v.c = ch;
        return v;
    }
    static View slice(View t, int off, int ch) {
        View v = t;
        v.coff = t.coff + off; v.c = ch;
        return v;
    }
    // one conv() unit of the reference; `out` must already have the right shape
    void conv(View in, View out, int filters, int k, bool down, int act, bool bn = true, const View* res = nullptr,
              bool upsample = false, bool out_f32 = false) {
        Layer L{};
        const int idx = (int)c.layers.size();
        L.d.idx = idx; L.d.ksize = k; L.d.stride = down ? 2 : 1; L.d.cin = in.c; L.d.cout = filters;
        L.d.act = act; L.d.has_bn = bn ? 1 : 0;
        L.in_h = in.h; L.in_w = in.w; L.out_h = down ? in.h / 2 : in.h; L.out_w = down ? in.w / 2 : in.w;
        const bool square = c.H == c.W;
        L.d.in_side = square ? L.in_h : -1; L.d.out_side = square ? L.out_h : -1;
        L.d.weight_offset = c.weight_floats;
        c.weight_floats += (bn ? 4 : 1) * (int64_t)filters + (int64_t)filters * in.c * k * k;
        c.flops_per_image += 2ll * k * k * in.c * filters * L.out_h * L.out_w;
        L.cout_pad = (int)round_up(filters, COUT_PAD);
        c.layers.push_back(L);
        Op op{};
        op.kind = idx == 0 ? OP_STEM : OP_CONV;
        op.conv = idx; op.in = in; op.out = out; op.upsample = upsample; op.out_f32 = out_f32;
        if (res) { op.res = *res; op.has_res = true; }
        snprintf(op.name, sizeof(op.name), "c%d", idx);
        c.ops.push_back(op);
    }
    View conv_new(View in, int filters, int k, bool down, int act) {
        View out = down ? alloc(in.h / 2, in.w / 2, filters) : alloc(in.h, in.w, filters);
        conv(in, out, filters, k, down, act);
        return out;
    }
    // csp_block (reference custom_layers.py:47-69): returns the [x, route] concat buffer
    View csp(View din, int width, int repeat, bool bottleneck) {
        View cat = alloc(din.h, din.w, 2 * width);
        // route conv (created first) and main-in conv read the same tensor: ONE GEMM with 2*width output
        // channels, [0,width) -> the route slice of the concat buffer, [width,2*width) -> x
        conv(din, slice(cat, width, width), width, 1, false, Y4_ACT_MISH);          // route
        View x = conv_new(din, width, 1, false, Y4_ACT_MISH);                        // main-in
        {
            Op second = c.ops.back(); c.ops.pop_back();
            Op& first = c.ops.back();
            first.conv2 = second.conv; first.out2 = second.out; first.split = width;
            snprintf(first.name, sizeof(first.name), "c%d+%d", first.conv, second.conv);
            Layer& L1 = c.layers[first.conv];
            Layer& L2 = c.layers[second.conv];
            L2.fused_with = first.conv; L2.fused_row = width;
            L1.extra_rows = width + COUT_PAD;      // partner rows + slack for its zero padding
        }
        for (int r = 0; r < repeat; ++r) {                                           // residual_block :34-44
            View t = conv_new(x, bottleneck ? width / 2 : width, 1, false, Y4_ACT_MISH);
            View x2 = alloc(din.h, din.w, width);
            conv(t, x2, width, 3, false, Y4_ACT_MISH, true, &x);                     // 3x3 + Add
            x = x2;
        }
        conv(x, slice(cat, 0, width), width, 1, false, Y4_ACT_MISH);                 // main-out
        return cat;
    }
    // the 5-conv PANet run (1x1, 3x3, 1x1, 3x3, 1x1); the last 1x1 writes into `last_out`
    View five(View x, int narrow, View last_out) {
        const int L = Y4_ACT_LEAKY;
        x = conv_new(x, narrow, 1, false, L);
        x = conv_new(x, narrow * 2, 3, false, L);
        x = conv_new(x, narrow, 1, false, L);
        x = conv_new(x, narrow * 2, 3, false, L);
        conv(x, last_out, narrow, 1, false, L);
        return last_out;
    }

    void build() {
        const int M = Y4_ACT_MISH, L = Y4_ACT_LEAKY;
        const int nout = 3 * (c.cfg.num_classes + 5);
        View img; img.buf = -1; img.h = c.H; img.w = c.W; img.cstride = 3; img.coff = 0; img.c = 3;     // caller's images
        // ---- cspdarknet53, reference custom_layers.py:100-138
        View x = conv_new(img, 32, 3, false, L);                 // c0  (leaky, as the reference)
        x = conv_new(x, 64, 3, true, L);                         // c1  (leaky, as the reference)
        x = csp(x, 64, 1, true);
        x = conv_new(x, 64, 1, false, M);
        x = conv_new(x, 128, 3, true, M);
        x = csp(x, 64, 2, false);
        x = conv_new(x, 128, 1, false, M);
        x = conv_new(x, 256, 3, true, M);
        x = csp(x, 128, 8, false);
        View route0 = x = conv_new(x, 256, 1, false, M);         // c37
        x = conv_new(x, 512, 3, true, M);
        x = csp(x, 256, 8, false);
        View route1 = x = conv_new(x, 512, 1, false, M);         // c58
        x = conv_new(x, 1024, 3, true, M);
        x = csp(x, 512, 4, false);
        x = conv_new(x, 1024, 1, false, M);                      // c71
        x = conv_new(x, 512, 1, false, L);
        x = conv_new(x, 1024, 3, false, L);
        View cat_spp = alloc(x.h, x.w, 2048);                     // [mp13 | mp9 | mp5 | x]
        conv(x, slice(cat_spp, 1536, 512), 512, 1, false, L);    // c74
        {
            Op op{};
            op.kind = OP_SPP; op.in = cat_spp; op.out = cat_spp;
            snprintf(op.name, sizeof(op.name), "spp");
            c.ops.push_back(op);
        }
        x = conv_new(cat_spp, 512, 1, false, L);
        x = conv_new(x, 1024, 3, false, L);
        View cat_bu2 = alloc(x.h, x.w, 1024);                     // [down(route1'') | route2]
        View route2 = slice(cat_bu2, 512, 512);
        conv(x, route2, 512, 1, false, L);                       // c77
        // ---- yolov4_neck, reference custom_layers.py:141-198
        View cat_td1 = alloc(route1.h, route1.w, 512);                 // [lateral(route1) | up(route2)]
        conv(route2, slice(cat_td1, 256, 256), 256, 1, false, L, true, nullptr, /*upsample=*/true);   // c78
        conv(route1, slice(cat_td1, 0, 256), 256, 1, false, L);                                       // c79
        View cat_bu1 = alloc(route1.h, route1.w, 512);                 // [down(route0') | route1']
        View route1p = five(cat_td1, 256, slice(cat_bu1, 256, 256));                                  // c80-c84
        View cat_td0 = alloc(route0.h, route0.w, 256);                 // [lateral(route0) | up(route1')]
        conv(route1p, slice(cat_td0, 128, 128), 128, 1, false, L, true, nullptr, /*upsample=*/true);  // c85
        conv(route0, slice(cat_td0, 0, 128), 128, 1, false, L);                                       // c86
        View route0p = five(cat_td0, 128, alloc(route0.h, route0.w, 128));                                   // c87-c91
        x = conv_new(route0p, 256, 3, false, L);                                                      // c92
        c.heads[0] = alloc(route0.h, route0.w, c.hcs, true); c.heads[0].c = nout;
        conv(x, c.heads[0], nout, 1, false, Y4_ACT_LINEAR, false, nullptr, false, true);              // c93
        conv(route0p, slice(cat_bu1, 0, 256), 256, 3, true, L);                                       // c94
        View route1pp = five(cat_bu1, 256, alloc(route1.h, route1.w, 256));                                  // c95-c99
        x = conv_new(route1pp, 512, 3, false, L);                                                     // c100
        c.heads[1] = alloc(route1.h, route1.w, c.hcs, true); c.heads[1].c = nout;
        conv(x, c.heads[1], nout, 1, false, Y4_ACT_LINEAR, false, nullptr, false, true);              // c101
        conv(route1pp, slice(cat_bu2, 0, 512), 512, 3, true, L);                                      // c102
        x = five(cat_bu2, 512, alloc(cat_bu2.h, cat_bu2.w, 512));                                             // c103-c107
        x = conv_new(x, 1024, 3, false, L);                                                           // c108
        c.heads[2] = alloc(cat_bu2.h, cat_bu2.w, c.hcs, true); c.heads[2].c = nout;
        conv(x, c.heads[2], nout, 1, false, Y4_ACT_LINEAR, false, nullptr, false, true);              // c109
    }
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

bool same_view(const View& a, const View& b) { return a.buf == b.buf && a.coff == b.coff && a.c == b.c; }

// does an op outside [lo, hi] read buffer `buf` (as its input or its residual)?
bool read_outside(const y4_ctx& c, int buf, int lo, int hi) {
    for (int k = 0; k < (int)c.ops.size(); ++k) {
        const Op& o = c.ops[k];
        if ((k < lo || k > hi) && (o.in.buf == buf || (o.has_res && o.res.buf == buf))) return true;
    }
    return false;
}

// Find the 3x3+Add -> 1x1 [-> 1x1 over Concatenate([., route])] runs of the plan that conv_chain.h can execute as one
// kernel (16-bit dtypes): head cout 64, Mish everywhere, tails 64 -> 64 and 128 -> 64|128.
void find_chains(y4_ctx& c) {
    if (c.cfg.dtype == Y4_F32) return;
    const int nops = (int)c.ops.size();
    auto in_chain = [&](int oi) {
        for (const Chain& ch : c.chains)
            if (ch.head == oi || ch.tail[0] == oi || ch.tail[1] == oi) return true;
        return false;
    };
    // LDS pairs whose tail is a fused CSP pair: the stride-2 3x3 conv that opens a stage -> that stage's route | main-in
    // 1x1 GEMM (custom_layers.py:107-108, :112-113 -> :58-60).  Found first: they save more traffic than the
    // split-head register chain that could start at the same CSP pair.
    for (int i = 0; i + 1 < nops; ++i) {
        const Op& a = c.ops[i];
        const Op& b = c.ops[i + 1];
        if (a.kind != OP_CONV || b.kind != OP_CONV || a.conv2 >= 0 || b.conv2 < 0) continue;
        const Layer& la = c.layers[a.conv];
        const Layer& lb = c.layers[b.conv];
        if ((la.d.cout != 128 && la.d.cout != 256) || a.upsample || a.out_f32 || a.has_res) continue;
        if (!(lb.d.ksize == 1 && lb.d.cin == la.d.cout && 2 * lb.d.cout == la.d.cout && b.split == lb.d.cout && !b.has_res &&
              same_view(b.in, a.out)))
            continue;
        Chain ch{i, {i + 1, -1}, read_outside(c, a.out.buf, i + 1, i + 1)};
        ch.lds_pair = true;
        c.chains.push_back(ch);
    }
    for (int i = 0; i + 1 < nops; ++i) {
        const Op& a = c.ops[i];
        const Op& b = c.ops[i + 1];
        if (in_chain(i) || in_chain(i + 1)) continue;
        if (a.kind == OP_CONV && b.kind == OP_CONV && a.conv2 >= 0 && b.conv2 < 0) {
            // fused CSP pair (64 + 64 rows over a 64-channel input) -> the 1x1 conv on its main-in half
            const Layer& la = c.layers[a.conv];
            const Layer& lb = c.layers[b.conv];
            if (la.d.ksize == 1 && la.d.cin % 64 == 0 && la.d.cout == 64 && a.split == 64 && la.d.act == Y4_ACT_MISH && !a.has_res &&
                lb.d.ksize == 1 && lb.d.cin == 64 && (lb.d.cout == 32 || lb.d.cout == 64) && lb.d.act == Y4_ACT_MISH && !b.has_res &&
                !b.upsample && !b.out_f32 && same_view(b.in, a.out2) && !c.layers[b.conv].has_tail) {
                Chain ch{i, {i + 1, -1}, true};          // both halves of the pair have later readers
                ch.lds_pair = true;
                c.chains.push_back(ch);
            }
            continue;
        }
        if (a.kind != OP_CONV || b.kind != OP_CONV || a.conv2 >= 0 || b.conv2 >= 0) continue;
        const Layer& la = c.layers[a.conv];
        const Layer& lb = c.layers[b.conv];
        if (!(la.d.ksize == 3 && la.d.stride == 1 && a.has_res && la.d.cout == 64 && la.d.act == Y4_ACT_MISH && !a.upsample)) continue;
        if (!(lb.d.ksize == 1 && lb.d.cin == 64 && lb.d.cout == 64 && lb.d.act == Y4_ACT_MISH && !b.has_res && !b.upsample &&
              !b.out_f32 && same_view(b.in, a.out)))
            continue;
        Chain ch{i, {i + 1, -1}, read_outside(c, a.out.buf, i + 1, i + 1)};
        if (i + 2 < nops) {
            const Op& d = c.ops[i + 2];
            if (d.kind == OP_CONV && d.conv2 < 0) {
                const Layer& ld = c.layers[d.conv];
                // d reads the whole concat buffer whose first 64 channels are b's output
                if (ld.d.ksize == 1 && ld.d.cin == 128 && (ld.d.cout == 64 || ld.d.cout == 128) && ld.d.act == Y4_ACT_MISH &&
                    !d.has_res && !d.upsample && !d.out_f32 && d.in.buf == b.out.buf && d.in.coff == 0 && b.out.coff == 0 &&
                    d.in.cstride == 128 && !read_outside(c, b.out.buf, i + 2, i + 2))
                    ch.tail[1] = i + 2;
            }
        }
        c.layers[b.conv].has_tail = true;
        if (ch.tail[1] >= 0) c.layers[c.ops[ch.tail[1]].conv].has_tail = true;
        c.chains.push_back(ch);
    }
    // alternatives (CFG 4): [1x1 64 -> 64] -> [1x1 over the concat, 128 -> 128] of every three-conv run above
    for (size_t ci = 0, nci = c.chains.size(); ci < nci; ++ci) {
        const Chain& pc = c.chains[ci];
        if (pc.lds_pair || pc.tail[1] < 0 || c.layers[c.ops[pc.tail[1]].conv].d.cout != 128) continue;
        Chain alt{pc.tail[0], {pc.tail[1], -1}, false};
        alt.alt_of = (int)ci;
        c.chains.push_back(alt);
    }
    // LDS pairs: conv (128 or 256 output channels) -> 1x1 conv with the same channel count reading exactly that output
    // (the residual blocks of the 76^2 and 38^2 stages: 3x3 + Add -> the next block's 1x1, custom_layers.py:34-44)
    for (int i = 0; i + 1 < nops; ++i) {
        const Op& a = c.ops[i];
        const Op& b = c.ops[i + 1];
        if (a.kind != OP_CONV || b.kind != OP_CONV || a.conv2 >= 0 || b.conv2 >= 0 || in_chain(i) || in_chain(i + 1)) continue;
        const Layer& la = c.layers[a.conv];
        const Layer& lb = c.layers[b.conv];
        if ((la.d.cout != 128 && la.d.cout != 256) || a.upsample || a.out_f32) continue;
        if (!(lb.d.ksize == 1 && lb.d.cin == la.d.cout && lb.d.cout <= la.d.cout && !b.has_res && !b.upsample && same_view(b.in, a.out)))
            continue;
        Chain ch{i, {i + 1, -1}, read_outside(c, a.out.buf, i + 1, i + 1)};
        ch.lds_pair = true;
        c.chains.push_back(ch);
    }
}

// The first CSP stage in the op list: [route|main-in pair (64+64 over 64)] [1x1 64->32] [3x3 32->64 + Add] [1x1 64->64]
// [1x1 128->64 over the concat], all Mish -- reference custom_layers.py:47-69 with residual_bottleneck=True, and :105.
void find_stage(y4_ctx& c) {
    if (c.cfg.dtype == Y4_F32) return;
    const int nops = (int)c.ops.size();
    for (int i = 0; i + 4 < nops; ++i) {
        const Op &a = c.ops[i], &b = c.ops[i + 1], &d = c.ops[i + 2], &e = c.ops[i + 3], &f = c.ops[i + 4];
        if (a.kind != OP_CONV || b.kind != OP_CONV || d.kind != OP_CONV || e.kind != OP_CONV || f.kind != OP_CONV) continue;
        if (a.conv2 < 0 || b.conv2 >= 0 || d.conv2 >= 0 || e.conv2 >= 0 || f.conv2 >= 0) continue;
        const Layer &la = c.layers[a.conv], &la2 = c.layers[a.conv2], &lb = c.layers[b.conv], &ld = c.layers[d.conv],
                    &le = c.layers[e.conv], &lf = c.layers[f.conv];
        auto mish1x1 = [](const Layer& l, int cin, int cout) {
            return l.d.ksize == 1 && l.d.cin == cin && l.d.cout == cout && l.d.act == Y4_ACT_MISH && l.d.has_bn;
        };
        if (!(mish1x1(la, 64, 64) && mish1x1(la2, 64, 64) && a.split == 64 && mish1x1(lb, 64, 32) && mish1x1(le, 64, 64) &&
              mish1x1(lf, 128, 64)))
            continue;
        if (!(ld.d.ksize == 3 && ld.d.stride == 1 && ld.d.cin == 32 && ld.d.cout == 64 && ld.d.act == Y4_ACT_MISH && d.has_res)) continue;
        // dataflow: b reads a's main-in half, d reads b and adds a's main-in half, e reads d, f reads [e | a's route half]
        if (!(same_view(b.in, a.out2) && same_view(d.in, b.out) && same_view(d.res, a.out2) && same_view(e.in, d.out))) continue;
        if (!(f.in.buf == e.out.buf && f.in.buf == a.out.buf && e.out.coff == f.in.coff && a.out.coff == f.in.coff + 64 && f.in.c == 128)) continue;
        if (a.upsample || f.upsample || f.out_f32 || !csp_stage_supported(c.cfg.dtype, a.in.h, a.in.w)) continue;
        // no other op may read the tensors that stop existing
        bool leak = false;
        for (int bufid : {a.out.buf, a.out2.buf, b.out.buf, d.out.buf}) leak = leak || read_outside(c, bufid, i, i + 4);
        if (leak) continue;
        c.stage_first = i; c.stage_last = i + 4;
        return;
    }
}

// residual_block (reference custom_layers.py:34-44) with filters1 == filters2 in {64, 128}: ops [1x1 C->C][3x3 C->C + Add(x)]
void find_resruns(y4_ctx& c) {
    if (c.cfg.dtype == Y4_F32) return;
    const int nops = (int)c.ops.size();
    for (int i = 0; i + 1 < nops; ++i) {
        const Op &a = c.ops[i], &b = c.ops[i + 1];
        if (a.kind != OP_CONV || b.kind != OP_CONV || a.conv2 >= 0 || b.conv2 >= 0 || a.has_res || !b.has_res) continue;
        const Layer &la = c.layers[a.conv], &lb = c.layers[b.conv];
        const int ch = la.d.cin;
        if (!resblock_supported(c.cfg.dtype, ch)) continue;
        if (!(la.d.ksize == 1 && la.d.cout == ch && la.d.act == Y4_ACT_MISH && la.d.has_bn && lb.d.ksize == 3 && lb.d.stride == 1 &&
              lb.d.cin == ch && lb.d.cout == ch && lb.d.act == Y4_ACT_MISH && lb.d.has_bn))
            continue;
        if (!(same_view(b.in, a.out) && same_view(b.res, a.in)) || a.upsample || b.upsample || a.out_f32 || b.out_f32) continue;
        if (read_outside(c, a.out.buf, i + 1, i + 1)) continue;      // the 1x1 conv's output must have no other reader
        c.resruns.push_back(ResRun{i, i + 1, ch});
    }
}

// Lifetime of every activation buffer in op-index time, for the aliasing layout.  A buffer lives from the first op that
// writes it to the last op that reads it; every group of ops that CAN run as one kernel (chains and LDS pairs, the stage
// kernel, residual blocks -- whether or not the tuner enables them) counts as one instant for everything it touches, because a
// fused kernel writes its tails' outputs while other workgroups of the same launch still read the head's inputs.  The raw
// heads live to the end (decode reads them; y4_get_heads).
static void buffer_lifetimes(const y4_ctx& c, std::vector<int>& first, std::vector<int>& last) {
    const int nb = (int)c.bufs.size(), nops = (int)c.ops.size();
    first.assign(nb, nops); last.assign(nb, -1);
    std::vector<int> lo(nops), hi(nops);                 // the instant [lo, hi] an op belongs to
    for (int i = 0; i < nops; ++i) lo[i] = hi[i] = i;
    auto merge = [&](int a, int b) {                     // ops a..b are one instant (merged with whatever they already belong to)
        int l = a, h = b;
        for (int i = a; i <= b; ++i) { l = std::min(l, lo[i]); h = std::max(h, hi[i]); }
        for (int i = l; i <= h; ++i) { lo[i] = std::min(lo[i], l); hi[i] = std::max(hi[i], h); }
    };
    for (const Chain& ch : c.chains) merge(ch.head, std::max(ch.tail[0], ch.tail[1]));
    if (c.stage_first >= 0) merge(c.stage_first, c.stage_last);
    for (const ResRun& r : c.resruns) merge(r.head, r.tail);
    if (nops > 1) merge(0, 1);                           // convs 0 + 1 (stem_down)
    for (int pass = 0; pass < 4; ++pass)                 // close the merge transitively (groups that overlap chain together)
        for (int i = 0; i < nops; ++i) merge(lo[i], hi[i]);
    auto touch = [&](const View& v, int i) {
        if (v.buf < 0) return;
        first[v.buf] = std::min(first[v.buf], lo[i]);
        last[v.buf] = std::max(last[v.buf], hi[i]);
    };
    for (int i = 0; i < nops; ++i) {
        const Op& o = c.ops[i];
        touch(o.in, i); touch(o.out, i);
        if (o.has_res) touch(o.res, i);
        if (o.conv2 >= 0) touch(o.out2, i);
    }
    for (int k = 0; k < 3; ++k) last[c.heads[k].buf] = nops;          // the raw heads outlive the forward
    if (c.retain_head_in)
        for (const Op& o : c.ops)
            if (o.out_f32) last[o.in.buf] = nops;                         // ... and so do their convs' inputs
    if (c.retain_block_in)
        for (const Op& o : c.ops)
            if (o.out_f32)
                for (const Op& q : c.ops)
                    if (q.kind == OP_CONV && q.out.buf == o.in.buf) last[q.in.buf] = nops;      // ... and the inputs of the convs in front
}

void layout(y4_ctx& c) {
    // ---- activations
    size_t off = 0;
    c.zero_off = off; off += ZERO_PAGE_BYTES;
    const size_t nb = (size_t)c.cfg.max_batch;
    for (auto& b : c.bufs) b.bytes = nb * b.h * b.w * b.channels * (b.f32 ? 4 : c.es);
    if (!c.alias_bufs) {
        for (auto& b : c.bufs) {
            b.offset = off;
            off = align256(off + b.bytes);
        }
    } else {
        // greedy interval colouring by size: the largest buffer first, each at the lowest offset where it does not overlap (in
        // memory) any already placed buffer whose lifetime intersects its own
        std::vector<int> first, last, order(c.bufs.size());
        buffer_lifetimes(c, first, last);
        for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return c.bufs[a].bytes != c.bufs[b].bytes ? c.bufs[a].bytes > c.bufs[b].bytes : a < b; });
        const size_t base = align256(off);
        size_t top = base;
        std::vector<int> placed;
        for (int bi : order) {
            Buffer& b = c.bufs[bi];
            size_t cand = base;
            for (bool moved = true; moved;) {
                moved = false;
                for (int pj : placed) {
                    const Buffer& o = c.bufs[pj];
                    const bool live_together = !(last[bi] < first[pj] || last[pj] < first[bi]);
                    if (live_together && cand < o.offset + align256(o.bytes) && o.offset < cand + align256(b.bytes)) {
                        cand = o.offset + align256(o.bytes);
                        moved = true;
                    }
                }
            }
            b.offset = cand;
            placed.push_back(bi);
            top = std::max(top, cand + align256(b.bytes));
        }
        off = top;
    }
    c.dbox_off = off; off = align256(off + nb * c.nbox * 16);
    c.cand_cap = (uint32_t)c.nbox * (uint32_t)c.cfg.num_classes;         // worst case: exact for any input
    c.keys_off = off; off = align256(off + nb * (size_t)c.cand_cap * 8);
    c.counts_off = off; off = align256(off + nb * 4 * COUNT_STRIDE);
    c.status_off = off; off = align256(off + 256);
    c.scratch_off = off; off = align256(off + nb * (size_t)c.cfg.max_total * 28 + nb * 4);
    c.splitk_off = off; off = align256(off + SPLITK_WS_BYTES);
    c.cells_per_img = 0;
    for (int i = 0; i < 3; ++i) { c.cell_base[i] = c.cells_per_img; c.cells_per_img += c.heads[i].h * c.heads[i].w; }
    c.obj_off = off; off = align256(off + nb * (size_t)c.cells_per_img * 16);
    c.act_bytes = off;
    // ---- weights
    off = 0;
    for (auto& L : c.layers) {
        const size_t rows = (size_t)L.cout_pad + L.extra_rows;
        const size_t wbytes = L.d.idx == 0 ? (size_t)8192 : rows * L.d.ksize * L.d.ksize * L.d.cin * c.es;
        L.w_off = off; off = align256(off + wbytes);
        L.scale_off = off; off = align256(off + rows * 4);
        L.shift_off = off; off = align256(off + rows * 4);
        if (L.has_tail) { L.tail_off = off; off = align256(off + (size_t)L.d.cout * L.d.cin * c.es); }
        L.has_frag = c.cfg.dtype != Y4_F32 && L.d.idx > 0 && L.d.ksize == 3 && L.d.stride == 1 && L.d.cin % 64 == 0 && L.fused_with < 0 && L.extra_rows == 0;
        if (L.has_frag) { L.frag_off = off; off = align256(off + wbytes); }
    }
    if (c.stage_first >= 0) { c.stage_blob_off = off; off = align256(off + csp_stage_blob_bytes()); }
    for (ResRun& r : c.resruns) { r.blob_off = off; off = align256(off + resblock_blob_bytes(r.c)); }
    c.wts_bytes = off;
}

int check_handle(y4_handle h) {
    Y4_REQUIRE(h != nullptr, Y4_EINVAL, "null handle");
    return Y4_OK;
}
// the preface of a setter: the events of an open timing session were laid out for the schedule it began with
int check_settable(y4_handle h, const char* who) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(h->t_max_steps == 0, Y4_ESTATE, "%s: a timing session is open", who);
    return Y4_OK;
}
// were the two handles created from the same configuration (the same plan, buffers of the same size)?
bool same_plan(const y4_ctx* a, const y4_ctx* b) {
    return a->ops.size() == b->ops.size() && a->chains.size() == b->chains.size() && a->resruns.size() == b->resruns.size() &&
           a->cfg.dtype == b->cfg.dtype && a->H == b->H && a->W == b->W && a->cfg.num_classes == b->cfg.num_classes &&
           a->cfg.max_batch == b->cfg.max_batch;
}
int check_ready(y4_handle h, int n) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(h->act && h->wts, Y4_ESTATE, "workspace not bound (call y4_bind_workspace first)");
    Y4_REQUIRE(h->weights_ready, Y4_ESTATE, "weights not packed (call y4_pack_weights first)");
    Y4_REQUIRE(n >= 1 && n <= h->cfg.max_batch, Y4_EINVAL, "batch %d outside [1, max_batch=%d]", n, h->cfg.max_batch);
    return Y4_OK;
}

char* buf_ptr(y4_handle h, const View& v, int img0 = 0) {
    const Buffer& b = h->bufs[v.buf];
    return h->act + b.offset + (size_t)img0 * b.h * b.w * b.channels * (b.f32 ? 4 : h->es);
}

// image `img0` of the caller's batch (float32 or uint8 elements, see y4_ctx::img_u8)
const void* img_at(y4_handle h, const void* imgs, int img0) {
    if (!imgs) return imgs;
    return (const char*)imgs + (size_t)img0 * h->H * h->W * 3 * (h->img_u8 ? 1 : 4);
}

struct Launch {
    int op, img0, cnt;
};
// execution schedule for a batch of n images (see y4_set_subbatch)
void build_schedule(y4_handle h, int n, std::vector<Launch>& out) {
    out.clear();
    const int nops = (int)h->ops.size();
    const Schedule& sc = h->sched;
    int first_full = 0;
    if (sc.sub_images > 0 && sc.sub_last_op >= 0 && n > sc.sub_images) {
        for (int img0 = 0; img0 < n; img0 += sc.sub_images)
            for (int i = 0; i <= sc.sub_last_op; ++i) out.push_back({i, img0, n - img0 < sc.sub_images ? n - img0 : sc.sub_images});
        first_full = sc.sub_last_op + 1;
    }
    for (int i = first_full; i < nops; ++i) out.push_back({i, 0, n});
}

// What op `oi` does under the handle's current switches: the one place that decides it (run_op executes the answer,
// y4_launch_counts counts it).  allow_chain = false (the tuner timing a conv as its own kernel): only the stem's fusion applies.
enum ExecKind { EX_SKIP, EX_SPP, EX_STEM, EX_STEM_DOWN, EX_RESBLOCK, EX_STAGE, EX_CHAIN, EX_LDS_PAIR, EX_ALT_CHAIN, EX_PLAIN };
struct OpExec {
    ExecKind kind;
    const ResRun* res = nullptr;      // EX_RESBLOCK
    const Chain* chain = nullptr;     // EX_CHAIN, EX_LDS_PAIR, EX_ALT_CHAIN
};
OpExec resolve_op(y4_handle h, int oi, bool allow_chain) {
    const Op& op = h->ops[oi];
    if (op.kind == OP_SPP) return {EX_SPP};
    if (op.kind == OP_STEM) return {h->sched.fuse_stem ? EX_STEM_DOWN : EX_STEM};
    if (h->sched.fuse_stem && op.conv == 1) return {EX_SKIP};                   // ran inside stem_down
    if (!allow_chain) return {EX_PLAIN};
    if (const ResRun* rr = h->res_of(oi, nullptr)) return h->heads_res(oi) ? OpExec{EX_RESBLOCK, rr} : OpExec{EX_SKIP};
    if (h->stage_active() && oi >= h->stage_first && oi <= h->stage_last) return {oi == h->stage_first ? EX_STAGE : EX_SKIP};
    const Chain* chain = nullptr;
    for (const Chain& ch : h->chains) {
        if (!h->chain_active(ch)) continue;     // (a head inside a residual-block kernel: its tails run alone or as the alternative run)
        if (ch.tail[0] == oi || ch.tail[1] == oi) return {EX_SKIP};       // ran with its head
        if (ch.head == oi) chain = &ch;
    }
    if (!chain) return {EX_PLAIN};
    return {chain->lds_pair ? EX_LDS_PAIR : chain->alt_of >= 0 ? EX_ALT_CHAIN : EX_CHAIN, nullptr, chain};
}

// A layer's packed weights and folded BN in the wts workspace.  A fused CSP pair shares one packed matrix: the partner's rows (and
// its scale / shift) follow the first conv's, at row `fused_row` of layer `fused_with`.
struct LayerW { char* w; float* scale; float* shift; };
static LayerW layer_w(y4_handle h, const Layer& L) {
    const Layer& D = L.fused_with >= 0 ? h->layers[L.fused_with] : L;
    const size_t row_bytes = (size_t)L.d.ksize * L.d.ksize * L.d.cin * h->es;
    return {h->wts + D.w_off + (size_t)L.fused_row * row_bytes, (float*)(h->wts + D.scale_off) + L.fused_row, (float*)(h->wts + D.shift_off) + L.fused_row};
}

// The kernels address their input through a raw buffer descriptor (2 GiB range, conv_igemm.hip): a batch whose input view is
// larger runs as consecutive image chunks (images are independent), `launch(first image, count)` each.  `reach`: what a 3x3
// conv's biased tap offsets add to the range (conv2d_launch's own check).  `fmt, args...` word the error; the bytes of one image
// are its last argument.
template <class F, class... A>
int for_image_chunks(y4_handle h, const View& in, int64_t reach, int n, int img0, const F& launch, const char* fmt, A... args) {
    const int64_t per_img = (int64_t)in.h * in.w * in.cstride * h->es;
    const int max_n = (int)(((1ll << 31) - 1 - reach) / per_img);
    if (max_n < 1) {
        set_error(fmt, args..., (long long)per_img);
        return Y4_EINVAL;
    }
    for (int i0 = 0; i0 < n; i0 += max_n)
        if (int r = launch(img0 + i0, n - i0 < max_n ? n - i0 : max_n)) return r;
    return Y4_OK;
}

int run_op(y4_handle h, int oi, const void* imgs, int n, hipStream_t s, int img0 = 0, bool allow_chain = true) {
    const Op& op = h->ops[oi];
    const OpExec ex = resolve_op(h, oi, allow_chain);
    switch (ex.kind) {
    case EX_SKIP:
        return Y4_OK;
    case EX_SPP:
        return spp_launch(h->cfg.dtype, buf_ptr(h, op.in, img0), n, op.in.h, op.in.w, op.in.cstride / 4, s);
    case EX_STEM_DOWN: {
        const Op& o1 = h->ops[1];
        const Layer &L = h->layers[0], &L1 = h->layers[1];
        const LayerW p = layer_w(h, L), p1 = layer_w(h, L1);
        return stem_down_launch(h->cfg.dtype, img_at(h, imgs, img0), h->img_u8 ? 1 : 0, n, h->H,      // (square only: y4_set_stem_fusion)
                                p.w, p.scale, p.shift, L.d.act, p1.w, p1.scale, p1.shift, L1.d.act,
                                buf_ptr(h, o1.out, img0), o1.out.cstride, o1.out.coff, s);
    }
    case EX_STEM: {
        const Layer& L = h->layers[0];
        const LayerW p = layer_w(h, L);
        return stem_conv_launch(h->cfg.dtype, img_at(h, imgs, img0), h->img_u8 ? 1 : 0, n, h->H, h->W, (const float*)p.w, p.scale, p.shift,
                                L.d.cout, L.d.act, buf_ptr(h, op.out, img0), op.out.cstride, op.out.coff, s);
    }
    case EX_RESBLOCK: {
        const Op& last = h->ops[ex.res->tail];
        auto launch = [&](int i0, int cnt) {
            return resblock_launch(h->cfg.dtype, ex.res->c, buf_ptr(h, op.in, i0), cnt, op.in.h, op.in.w, op.in.cstride, op.in.coff,
                                   h->wts + ex.res->blob_off, buf_ptr(h, last.out, i0), last.out.cstride, last.out.coff, s);
        };
        return for_image_chunks(h, op.in, 0, n, img0, launch,
                                "residual block: one image of the input view (%lld B) exceeds the 2 GiB buffer range");
    }
    case EX_STAGE: {
        const Op& last = h->ops[h->stage_last];
        auto launch = [&](int i0, int cnt) {
            return csp_stage_launch(h->cfg.dtype, buf_ptr(h, op.in, i0), cnt, op.in.h, op.in.w, op.in.cstride, op.in.coff,
                                    h->wts + h->stage_blob_off, buf_ptr(h, last.out, i0), last.out.cstride, last.out.coff, s);
        };
        return for_image_chunks(h, op.in, 0, n, img0, launch,
                                "stage kernel: one image of the input view (%lld B) exceeds the 2 GiB buffer range");
    }
    case EX_PLAIN: case EX_CHAIN: case EX_LDS_PAIR: case EX_ALT_CHAIN:
        break;
    }
    // the conv family: one conv2d_launch, carrying the run's tails when op heads one
    const Layer& L = h->layers[op.conv];
    const LayerW lw = layer_w(h, L);
    const Chain* chain = ex.chain;
    auto launch = [&](int i0, int cnt) -> int {
        y4_conv_desc d{};
        d.dtype = h->cfg.dtype;
        d.n = cnt; d.h = op.in.h; d.w = op.in.w; d.cin = op.in.c;
        d.cout = op.conv2 >= 0 ? 2 * L.d.cout : L.d.cout; d.ksize = L.d.ksize; d.stride = L.d.stride; d.act = L.d.act;
        d.upsample = op.upsample ? 1 : 0; d.out_f32 = op.out_f32 ? 1 : 0;
        d.in_cstride = op.in.cstride; d.in_coff = op.in.coff;
        d.out_cstride = op.out.cstride; d.out_coff = op.out.coff;
        d.in = buf_ptr(h, op.in, i0); d.wt = lw.w; d.scale = lw.scale; d.shift = lw.shift;
        d.wt_frag = L.has_frag ? h->wts + L.frag_off : nullptr;
        d.out = buf_ptr(h, op.out, i0);
        if (op.has_res) { d.res = buf_ptr(h, op.res, i0); d.res_cstride = op.res.cstride; d.res_coff = op.res.coff; }
        if (op.conv2 >= 0) { d.out2 = buf_ptr(h, op.out2, i0); d.out2_cstride = op.out2.cstride; d.out2_coff = op.out2.coff; d.split = op.split; }
        d.tile = chain ? h->sched.run[chain - h->chains.data()].tile : h->sched.tile[oi];
        d.splitk_ws = h->act + h->splitk_off; d.splitk_ws_bytes = SPLITK_WS_BYTES;
        // a float32 head (as a plain launch or as the tail of an LDS pair) also fills its cells' slots of the objectness array
        ConvObjDesc od{};
        const ConvObjDesc* odp = nullptr;
        int obj_head = -1;
        {
            const Op* ho = op.out_f32 ? &op : (ex.kind == EX_LDS_PAIR && h->ops[chain->tail[0]].out_f32 ? &h->ops[chain->tail[0]] : nullptr);
            if (ho)
                for (int i = 0; i < 3; ++i)
                    if (h->heads[i].buf == ho->out.buf) {
                        od.obj = (float*)(h->act + h->obj_off) + (size_t)i0 * h->cells_per_img * 4;
                        od.nf = 5 + h->cfg.num_classes; od.cells_per_img = h->cells_per_img; od.cell_base = h->cell_base[i];
                        odp = &od;
                        obj_head = i;
                        h->obj_n[i] = -1;                     // (valid again once the launch below has been enqueued)
                    }
        }
        auto launched = [&](int rc) {                          // the side array counts only after a successful enqueue
            if (rc == Y4_OK && obj_head >= 0) h->obj_n[obj_head] = i0 + cnt;
            return rc;
        };
        if (ex.kind == EX_LDS_PAIR) {
            const Op& to = h->ops[chain->tail[0]];
            const Layer& TL = h->layers[to.conv];
            const LayerW tw = layer_w(h, TL);
            ConvPairDesc pd{};
            pd.w = tw.w; pd.scale = tw.scale; pd.shift = tw.shift;
            pd.act = TL.d.act; pd.cout = TL.d.cout; pd.out_f32 = to.out_f32 ? 1 : 0; pd.store_x = h->stores_x(*chain) ? 1 : 0;
            pd.fin = buf_ptr(h, to.out, i0); pd.fin_cstride = to.out.cstride; pd.fin_coff = to.out.coff;
            if (to.conv2 >= 0) {          // the tail is a fused CSP pair: both convs' rows, split over two views
                pd.cout = 2 * TL.d.cout; pd.split = to.split;
                pd.fin2 = buf_ptr(h, to.out2, i0); pd.fin2_cstride = to.out2.cstride; pd.fin2_coff = to.out2.coff;
            }
            return launched(conv2d_launch(&d, h->act + h->zero_off, s, nullptr, &pd, odp));
        }
        if (ex.kind == EX_ALT_CHAIN) {
            // this op (64 -> 64) feeds the conv over Concatenate([its output, route]) in registers; its own output is not stored
            const Op& to = h->ops[chain->tail[0]];
            const Layer& TL = h->layers[to.conv];
            ConvChainDesc cd{};
            cd.ntail = 2; cd.concat_only = 1; cd.store_x = 0;
            const LayerW tw = layer_w(h, TL);
            cd.tail[1].w = h->wts + TL.tail_off; cd.tail[1].scale = tw.scale; cd.tail[1].shift = tw.shift;
            cd.tail[1].cout = TL.d.cout;
            cd.tail[1].src2 = buf_ptr(h, to.in, i0);
            cd.tail[1].src2_cstride = to.in.cstride;
            cd.tail[1].src2_coff = to.in.coff + 64;
            cd.fin = buf_ptr(h, to.out, i0); cd.fin_cstride = to.out.cstride; cd.fin_coff = to.out.coff;
            return conv2d_launch(&d, h->act + h->zero_off, s, &cd);
        }
        if (ex.kind == EX_CHAIN) {
            ConvChainDesc cd{};
            cd.store_x = h->stores_x(*chain) ? 1 : 0;
            const Op* last = &op;
            for (int t = 0; t < 2 && chain->tail[t] >= 0; ++t) {
                const Op& to = h->ops[chain->tail[t]];
                const Layer& TL = h->layers[to.conv];
                const LayerW tw = layer_w(h, TL);
                cd.tail[t].w = h->wts + TL.tail_off; cd.tail[t].scale = tw.scale; cd.tail[t].shift = tw.shift;
                cd.tail[t].cout = TL.d.cout;
                if (t == 1) {                       // the concat partner: channels [64, 128) of the buffer the first tail writes into
                    cd.tail[t].src2 = buf_ptr(h, to.in, i0);
                    cd.tail[t].src2_cstride = to.in.cstride;
                    cd.tail[t].src2_coff = to.in.coff + 64;
                }
                cd.ntail = t + 1;
                last = &to;
            }
            cd.fin = buf_ptr(h, last->out, i0); cd.fin_cstride = last->out.cstride; cd.fin_coff = last->out.coff;
            return conv2d_launch(&d, h->act + h->zero_off, s, &cd);
        }
        return launched(conv2d_launch(&d, h->act + h->zero_off, s, nullptr, nullptr, odp));
    };
    const int64_t reach = L.d.ksize == 3 ? ((int64_t)3 * op.in.w + 3) * op.in.cstride * h->es + (int64_t)op.in.c * h->es : 0;
    return for_image_chunks(h, op.in, reach, n, img0, launch,
                            "conv %d: one image's input (%lld B) exceeds the 2 GiB buffer-descriptor range", op.conv);
}

// A candidate store: what the decode stage fills and an NMS or a gather reads -- the workspace's, one list per batch row, or a
// gather scratch's, one list per group (y4_nms_gathered)
struct CandStore {
    float* dboxes;                   // [rows, nbox, 4]
    unsigned long long* keys;        // [rows, cap]
    uint32_t* counts;                // [rows * COUNT_STRIDE]
    uint32_t cap;
    int nbox;
    uint32_t* status;                // the handle's overflow word
    FastDiv div_c;
};
CandStore cand_store(y4_handle h, float* dboxes, unsigned long long* keys, uint32_t* counts, uint32_t cap, int nbox) {
    return CandStore{dboxes, keys, counts, cap, nbox, (uint32_t*)(h->act + h->status_off), fastdiv_make((uint32_t)h->cfg.num_classes)};
}
CandStore workspace_cands(y4_handle h) {
    return cand_store(h, (float*)(h->act + h->dbox_off), (unsigned long long*)(h->act + h->keys_off), (uint32_t*)(h->act + h->counts_off),
                      h->cand_cap, h->nbox);
}

int run_decode(y4_handle h, int n, float score_thr, hipStream_t s) {
    const y4_config& cfg = h->cfg;
    const CandStore c = workspace_cands(h);
    DecodeK k{};
    int off = 0, cells = 0;
    for (int i = 0; i < 3; ++i) {
        k.head[i] = (const float*)buf_ptr(h, h->heads[i]);
        k.gh[i] = h->heads[i].h; k.gw[i] = h->heads[i].w; k.stride[i] = cfg.strides[i]; k.box_off[i] = off;
        off += 3 * k.gh[i] * k.gw[i]; cells += k.gh[i] * k.gw[i];
        k.xyscale[i] = cfg.xyscale[i];
        k.xyoff[i] = (float)(0.5 * ((double)cfg.xyscale[i] - 1.0));
    }
    memcpy(k.anchors, cfg.anchors, sizeof(k.anchors));
    k.cells_per_img = cells; k.N = n; k.C = cfg.num_classes; k.hcs = h->hcs; k.nbox = c.nbox;
    k.div_cells = fastdiv_make((uint32_t)cells);
    for (int i = 0; i < 3; ++i) k.div_gw[i] = fastdiv_make((uint32_t)k.gw[i]);
    k.img_h = (float)h->H; k.img_w = (float)h->W; k.score_thr = score_thr;
    k.dboxes = c.dboxes; k.keys = c.keys; k.counts = c.counts; k.cap = c.cap;
    k.obj = h->obj_n[0] >= n && h->obj_n[1] >= n && h->obj_n[2] >= n ? (const float*)(h->act + h->obj_off) : nullptr;
    if (int r = decode_launch(k, s, h->counts_clean ? 0 : cfg.max_batch)) return r;
    h->counts_clean = false;                          // ... until this decode's NMS (or gather) has been enqueued behind it
    h->counts_n = n;
    return Y4_OK;
}

struct NmsOutputs { float* boxes; float* scores; float* classes; int32_t* valid; int32_t* kept_idx; };
// NMS of the first n lists of a candidate store under the handle's rule and caps.  box_map: [n][4] per list, applied in the
// output stage (y4_decode_nms_mapped), or null
int nms_over(y4_handle h, const CandStore& c, int n, float iou_thr, const NmsOutputs& o, const float* box_map, hipStream_t s) {
    const y4_config& cfg = h->cfg;
    NmsK k{};
    k.dboxes = c.dboxes; k.keys = c.keys; k.counts = c.counts; k.cap = c.cap;
    k.N = n; k.C = cfg.num_classes; k.nbox = c.nbox;
    k.max_total = cfg.max_total; k.max_per_class = cfg.max_per_class; k.iou_thr = iou_thr;
    k.out_boxes = o.boxes; k.out_scores = o.scores; k.out_classes = o.classes; k.out_valid = o.valid; k.out_idx = o.kept_idx;
    k.status = c.status; k.div_c = c.div_c;
    k.box_map = box_map;
    k.kind = h->nms_kind; k.beta = h->nms_beta; k.agnostic = h->nms_agnostic;
    // the decay mode that is on: matrix, else soft, else none -- its kernel over the same lists into the same outputs
    const DecayMode& m = h->matrix.method != 0 ? h->matrix : h->soft;
    if (m.method == 0) return nms_launch(k, s);
    const DecayK dk{m.method, m.sigma, m.min_score < 0.f ? cfg.score_threshold : m.min_score, m.top_k};
    return &m == &h->matrix ? matrix_nms_launch(k, dk, s) : soft_nms_launch(k, dk, s);
}

// ... of the workspace's lists, behind run_decode
int run_nms(y4_handle h, int n, float iou_thr, const NmsOutputs& o, const float* box_map, hipStream_t s) {
    if (int r = nms_over(h, workspace_cands(h), n, iou_thr, o, box_map, s)) return r;
    h->counts_clean = h->counts_n <= n;               // (an NMS over fewer images than were decoded leaves counters behind)
    return Y4_OK;
}

// Merge-NMS behind an NMS of the same lists: every kept box becomes the score-weighted mean of the candidates it absorbed
// (box_merge.hip).  counts_dev: [n] the lists' raw counts, saved before nms_kernel zeroed the counters
int merge_over(y4_handle h, const CandStore& c, int n, float iou_thr, const NmsOutputs& o, const int32_t* counts_dev, const float* box_map,
               hipStream_t s) {
    MergeK k{};
    k.dboxes = c.dboxes; k.keys = c.keys; k.counts = counts_dev; k.cap = c.cap;
    k.N = n; k.C = h->cfg.num_classes; k.nbox = c.nbox; k.max_total = h->cfg.max_total; k.iou_thr = iou_thr;
    k.out_boxes = o.boxes; k.out_scores = o.scores; k.out_classes = o.classes; k.out_valid = o.valid; k.out_idx = o.kept_idx;
    k.div_c = c.div_c;
    k.box_map = box_map;
    k.kind = h->nms_kind; k.beta = h->nms_beta; k.agnostic = h->nms_agnostic;
    return box_merge_launch(k, s);
}

// The detection tail of every entry point: [decode ->] [save the lists' counts ->] NMS [-> merge], on one stream in this order.
// gathered: the lists of a gather scratch (y4_nms_gathered*), which are there already; null: the workspace's lists, decoded here
// (decoded: an event to record behind the decode, or null) and under run_nms's counter bookkeeping.  A threshold < 0 is the config's.
enum { TAIL_COUNTS = 1, TAIL_MERGE = 2 };      // cand_count <- the raw counts, before the NMS zeroes the counters | merge_over behind
int detect_tail(y4_handle h, const char* who, const CandStore* gathered, int n, float iou_threshold, float score_threshold, int flags,
                int32_t* cand_count, const NmsOutputs& o, const float* box_map, hipStream_t s, hipEvent_t decoded = nullptr) {
    const CandStore c = gathered ? *gathered : workspace_cands(h);
    Y4_REQUIRE(!(flags & TAIL_MERGE) || c.cap < MERGE_MAX_CAP, Y4_EINVAL, "%s: a list capacity of %u keys is not below the 2^25 the merge allows",
               who, c.cap);
    const float iou = iou_threshold < 0.f ? h->cfg.iou_threshold : iou_threshold;
    if (!gathered) {
        if (int r = run_decode(h, n, score_threshold < 0.f ? h->cfg.score_threshold : score_threshold, s)) return r;
        if (decoded) Y4_CHECK_HIP(hipEventRecord(decoded, s));
    }
    if (flags & TAIL_COUNTS)
        if (int r = gather_counts_launch(c.counts, cand_count, n, s)) return r;
    if (int r = gathered ? nms_over(h, c, n, iou, o, box_map, s) : run_nms(h, n, iou, o, box_map, s)) return r;
    return flags & TAIL_MERGE ? merge_over(h, c, n, iou, o, cand_count, box_map, s) : Y4_OK;
}

}  // namespace

extern "C" {

const char* y4_last_error(void) { return g_err; }
const char* y4_version(void) { return "yolo4hip 0.5.1 (gfx950)"; }

int y4_create(const y4_config* cfg, y4_handle* out) {
    Y4_REQUIRE(cfg && out, Y4_EINVAL, "y4_create: null argument");
    return y4_create_hw(cfg, cfg->img_size, cfg->img_size, out);
}

int y4_create_hw(const y4_config* cfg, int32_t img_h, int32_t img_w, y4_handle* out) {
    Y4_REQUIRE(cfg && out, Y4_EINVAL, "y4_create_hw: null argument");
    // the reference's asserts (models.py:24,38), for each side; the reference's 'not support yet' for H != W is lifted
    Y4_REQUIRE(img_h > 0 && img_h % 32 == 0 && img_w > 0 && img_w % 32 == 0, Y4_EINVAL,
               "img_size %d x %d: each side must be a positive multiple of the last stride (32)", img_h, img_w);
    Y4_REQUIRE(cfg->num_classes > 0, Y4_EINVAL, "no classes detected!");
    Y4_REQUIRE(cfg->num_classes <= 4096, Y4_EINVAL, "num_classes %d too large", cfg->num_classes);
    Y4_REQUIRE(cfg->max_batch >= 1, Y4_EINVAL, "max_batch %d", cfg->max_batch);
    Y4_REQUIRE(cfg->dtype >= Y4_F32 && cfg->dtype <= Y4_F16, Y4_EINVAL, "dtype %d", cfg->dtype);
    Y4_REQUIRE(cfg->strides[0] == 8 && cfg->strides[1] == 16 && cfg->strides[2] == 32, Y4_EINVAL,
               "strides must be 8,16,32 (they are fixed by the graph)");
    Y4_REQUIRE(cfg->max_total >= 1 && cfg->max_total <= 1024 && cfg->max_per_class >= 1, Y4_EINVAL, "max_total/max_per_class");
    y4_ctx* c = new y4_ctx();
    c->cfg = *cfg;
    c->cfg.img_size = img_h == img_w ? img_h : -1;    // (a rectangle has no one side: H and W below)
    c->es = elem_size(cfg->dtype);
    c->H = img_h; c->W = img_w;
    c->hcs = (int)round_up(3 * (cfg->num_classes + 5), 8);
    c->nbox = 0;
    for (int i = 0; i < 3; ++i) c->nbox += 3 * (c->H / cfg->strides[i]) * (c->W / cfg->strides[i]);
    if ((int64_t)c->nbox * cfg->num_classes >= (1ll << 31)) {
        delete c;
        set_error("num_boxes*num_classes overflows the 32-bit candidate id");
        return Y4_EINVAL;
    }
    Builder(*c).build();
    find_chains(*c);
    find_stage(*c);
    find_resruns(*c);
    c->sched.tile.assign(c->ops.size(), 0);
    c->sched.run.assign(c->chains.size(), Schedule::Run{});
    layout(*c);
    *out = c;
    return Y4_OK;
}

int y4_destroy(y4_handle h) {
    delete h;
    return Y4_OK;
}

int y4_num_layers(y4_handle h) { return h ? (int)h->layers.size() : Y4_EINVAL; }

int y4_layer_info(y4_handle h, int idx, y4_layer_desc* out) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(out && idx >= 0 && idx < (int)h->layers.size(), Y4_EINVAL, "layer index %d", idx);
    *out = h->layers[idx].d;
    return Y4_OK;
}

int y4_input_dims(y4_handle h, int32_t* img_h, int32_t* img_w) {
    if (int r = check_handle(h)) return r;
    if (img_h) *img_h = h->H;
    if (img_w) *img_w = h->W;
    return Y4_OK;
}

int y4_layer_dims(y4_handle h, int idx, int32_t dims[4]) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(dims && idx >= 0 && idx < (int)h->layers.size(), Y4_EINVAL, "layer index %d", idx);
    const Layer& L = h->layers[idx];
    dims[0] = L.in_h; dims[1] = L.in_w; dims[2] = L.out_h; dims[3] = L.out_w;
    return Y4_OK;
}

int y4_model_info(y4_handle h, int64_t* flops_per_image, int32_t* num_boxes, int32_t* head_cstride, int64_t* weight_floats) {
    if (int r = check_handle(h)) return r;
    if (flops_per_image) *flops_per_image = h->flops_per_image;
    if (num_boxes) *num_boxes = h->nbox;
    if (head_cstride) *head_cstride = h->hcs;
    if (weight_floats) *weight_floats = h->weight_floats;
    return Y4_OK;
}

int y4_set_workspace_aliasing(y4_handle h, int on) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(!h->act, Y4_ESTATE, "y4_set_workspace_aliasing: the workspace is already bound (call it before y4_workspace_bytes / y4_bind_workspace)");
    Y4_REQUIRE(!(on && h->sched.sub_images > 0), Y4_ESTATE, "y4_set_workspace_aliasing: not together with sub-batching");
    h->alias_bufs = on != 0;
    layout(*h);
    return Y4_OK;
}

int y4_workspace_bytes(y4_handle h, size_t* act_bytes, size_t* wts_bytes) {
    if (int r = check_handle(h)) return r;
    if (act_bytes) *act_bytes = h->act_bytes;
    if (wts_bytes) *wts_bytes = h->wts_bytes;
    return Y4_OK;
}

// Does the forward write conv `conv_idx`'s output view under the current switches?  Not while a fused kernel keeps it on chip: conv 0
// under stem fusion, convs 2 .. 6 under the stage kernel, the 1x1 conv of a residual-block kernel, and inside a run that executes as
// one kernel everything but its last tail and -- where it has other readers (stores_x) -- its head.
static bool conv_materialised(y4_handle h, int oi, int conv_idx) {
    if (h->sched.fuse_stem && conv_idx == 0) return false;
    if (h->stage_active() && oi >= h->stage_first && oi < h->stage_last) return false;
    if (h->heads_res(oi)) return false;
    for (const Chain& ch : h->chains) {
        if (!h->chain_active(ch) || resolve_op(h, ch.head, true).chain != &ch) continue;
        if (ch.head == oi && (ch.alt_of >= 0 || !h->stores_x(ch))) return false;
        if (ch.tail[0] == oi && ch.tail[1] >= 0) return false;
    }
    return true;
}

// The regions layout() placed, sorted by offset (ACT rows of an aliased layout share bytes; rows at one offset: the larger first).
static void workspace_rows(const y4_ctx& c, std::vector<y4_workspace_row>& rows) {
    rows.clear();
    auto add = [&](const char* name, int kind, size_t off, size_t bytes, size_t image_bytes, int buf = -1, int first = -1, int last = -1) {
        y4_workspace_row r{};
        snprintf(r.name, sizeof(r.name), "%s", name);
        r.kind = kind; r.buffer = buf; r.first_op = first; r.last_op = last;
        r.offset = off; r.bytes = bytes; r.image_bytes = image_bytes;
        rows.push_back(r);
    };
    const size_t nb = (size_t)c.cfg.max_batch;
    std::vector<int> first, last;
    buffer_lifetimes(c, first, last);
    add("zero_page", Y4_WS_ZERO, c.zero_off, ZERO_PAGE_BYTES, 0);
    for (size_t i = 0; i < c.bufs.size(); ++i) {
        char name[16];
        snprintf(name, sizeof(name), "act%zu", i);
        add(name, Y4_WS_ACT, c.bufs[i].offset, c.bufs[i].bytes, c.bufs[i].bytes / nb, (int)i, first[i], last[i]);
    }
    add("boxes", Y4_WS_TAIL, c.dbox_off, nb * c.nbox * 16, (size_t)c.nbox * 16);
    add("keys", Y4_WS_TAIL, c.keys_off, nb * (size_t)c.cand_cap * 8, (size_t)c.cand_cap * 8);
    add("counts", Y4_WS_ZERO, c.counts_off, nb * 4 * COUNT_STRIDE, 4 * COUNT_STRIDE);
    add("status", Y4_WS_ZERO, c.status_off, 256, 0);
    // (y4_profile's outputs: five arrays packed for the n of the call, so no fixed bytes per image)
    add("nms_scratch", Y4_WS_TAIL, c.scratch_off, nb * (size_t)c.cfg.max_total * 28 + nb * 4, 0);
    add("splitk_counters", Y4_WS_ZERO, c.splitk_off, SPLITK_CNT_BYTES, 0);
    add("splitk_partials", Y4_WS_SCRATCH, c.splitk_off + SPLITK_CNT_BYTES, SPLITK_WS_BYTES - SPLITK_CNT_BYTES, 0);
    add("objectness", Y4_WS_TAIL, c.obj_off, nb * (size_t)c.cells_per_img * 16, (size_t)c.cells_per_img * 16);
    std::stable_sort(rows.begin(), rows.end(), [](const y4_workspace_row& a, const y4_workspace_row& b) {
        return a.offset != b.offset ? a.offset < b.offset : a.bytes > b.bytes;
    });
}

int y4_workspace_map(y4_handle h, y4_workspace_row* rows_out, int capacity, int* count_out) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(count_out && capacity >= 0 && (rows_out || capacity == 0), Y4_EINVAL, "y4_workspace_map: null argument");
    std::vector<y4_workspace_row> rows;
    workspace_rows(*h, rows);
    *count_out = (int)rows.size();
    for (int i = 0; i < capacity && i < (int)rows.size(); ++i) rows_out[i] = rows[i];
    return Y4_OK;
}

int y4_conv_output_view(y4_handle h, int conv_idx, int32_t* row, int32_t* channel_offset, int32_t* channel_stride, int32_t* materialised) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(row && channel_offset && channel_stride, Y4_EINVAL, "y4_conv_output_view: null argument");
    for (const Op& op : h->ops) {
        if (op.kind == OP_SPP || (op.conv != conv_idx && op.conv2 != conv_idx)) continue;
        const View& v = op.conv == conv_idx ? op.out : op.out2;
        std::vector<y4_workspace_row> rows;
        workspace_rows(*h, rows);
        for (size_t i = 0; i < rows.size(); ++i)
            if (rows[i].kind == Y4_WS_ACT && rows[i].buffer == v.buf) {
                *row = (int32_t)i; *channel_offset = v.coff; *channel_stride = v.cstride;
                if (materialised) *materialised = conv_materialised(h, (int)(&op - h->ops.data()), conv_idx) ? 1 : 0;
                return Y4_OK;
            }
    }
    set_error("no conv with index %d", conv_idx);
    return Y4_EINVAL;
}

int y4_bind_workspace(y4_handle h, void* act_dev, size_t act_bytes, void* wts_dev, size_t wts_bytes) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(act_dev && wts_dev, Y4_EINVAL, "y4_bind_workspace: null workspace");
    Y4_REQUIRE(((uintptr_t)act_dev & 255) == 0 && ((uintptr_t)wts_dev & 255) == 0, Y4_EINVAL, "workspaces must be 256-byte aligned");
    Y4_REQUIRE(act_bytes >= h->act_bytes, Y4_ENOMEM, "act workspace %zu < %zu bytes", act_bytes, h->act_bytes);
    Y4_REQUIRE(wts_bytes >= h->wts_bytes, Y4_ENOMEM, "wts workspace %zu < %zu bytes", wts_bytes, h->wts_bytes);
    h->act = (char*)act_dev;
    h->counts_clean = false;
    h->wts = (char*)wts_dev;
    h->weights_ready = false;
    // The WHOLE activation workspace starts as zeros (round 5; once per bind, ~1 ms per 3 GB): the zero page, the NMS status word and
    // the split-K tile counters (zero between launches) need it, and no result can then depend on what the caller's memory held
    // before -- a workspace from a caching allocator carries the previous owner's tensors.  The previous owner's WORK too: kernels still
    // pending on some non-blocking stream against the recycled block would land after a null-stream memset, so the
    // device is drained first -- binding is an init-time call.
    Y4_CHECK_HIP(hipDeviceSynchronize());
    Y4_CHECK_HIP(hipMemset(h->act, 0, h->act_bytes));
    // ... and it HAS happened when this returns: the caller may use the handle on any stream next, and a non-blocking stream (every
    // torch.cuda.Stream is one) does not order itself behind the null stream the memset ran on
    Y4_CHECK_HIP(hipStreamSynchronize(nullptr));
    return Y4_OK;
}

int y4_pack_weights(y4_handle h, const float* blob, size_t n_floats, void* stream) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(h->act && h->wts, Y4_ESTATE, "workspace not bound (call y4_bind_workspace first)");
    Y4_REQUIRE(blob, Y4_EINVAL, "y4_pack_weights: null blob");
    Y4_REQUIRE((int64_t)n_floats >= h->weight_floats, Y4_EINVAL, "weight blob has %zu floats, the plan needs %lld",
               n_floats, (long long)h->weight_floats);
    hipStream_t s = (hipStream_t)stream;
    for (const Layer& L : h->layers) {
        const float* rec = blob + L.d.weight_offset;
        const float* w = rec + (L.d.has_bn ? 4 : 1) * (int64_t)L.d.cout;
        const LayerW p = layer_w(h, L);                    // (a fused CSP pair's partner: its rows of the first conv's matrix)
        if (int r = fold_bn_launch(rec, p.scale, p.shift, L.d.cout, L.cout_pad, L.d.has_bn, s)) return r;
        if (L.d.idx == 0) {
            if (int r = pack_stem_weights(w, (float*)p.w, L.d.cout, s)) return r;
        } else {
            if (int r = pack_conv_weights(h->cfg.dtype, L.d.cout, L.d.cin, L.d.ksize, w, p.w, s)) return r;
            if (L.has_tail)
                if (int r = pack_tail_weights(h->cfg.dtype, L.d.cout, L.d.cin, w, h->wts + L.tail_off, s)) return r;
            if (L.has_frag)
                if (int r = pack_conv_frag32(h->cfg.dtype, L.d.cout, L.d.cin, p.w, h->wts + L.frag_off, s)) return r;
        }
    }
    if (h->stage_first >= 0) {
        // convs 2..7 once more, as the fragment-ordered blob of csp_stage_kernel (same rounding of the same floats)
        const Op& a = h->ops[h->stage_first];
        const int convs[6] = {a.conv, a.conv2, h->ops[h->stage_first + 1].conv, h->ops[h->stage_first + 2].conv,
                              h->ops[h->stage_first + 3].conv, h->ops[h->stage_first + 4].conv};
        const float *w[6], *sc[6], *sh[6];
        for (int k = 0; k < 6; ++k) {
            const Layer& L = h->layers[convs[k]];
            const LayerW p = layer_w(h, L);
            w[k] = blob + L.d.weight_offset + 4 * (int64_t)L.d.cout;
            sc[k] = p.scale; sh[k] = p.shift;
        }
        if (int r = pack_csp_stage(h->cfg.dtype, w, sc, sh, h->wts + h->stage_blob_off, s)) return r;
    }
    for (const ResRun& r : h->resruns) {
        const Layer &L1 = h->layers[h->ops[r.head].conv], &L3 = h->layers[h->ops[r.tail].conv];
        const LayerW p1 = layer_w(h, L1), p3 = layer_w(h, L3);
        if (int rc = pack_resblock(h->cfg.dtype, r.c, blob + L1.d.weight_offset + 4 * (int64_t)L1.d.cout, p1.scale, p1.shift,
                                   blob + L3.d.weight_offset + 4 * (int64_t)L3.d.cout, p3.scale, p3.shift, h->wts + r.blob_off, s))
            return rc;
    }
    h->weights_ready = true;
    return Y4_OK;
}

int y4_adopt_packed_weights(y4_handle h) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(h->act && h->wts, Y4_ESTATE, "workspace not bound (call y4_bind_workspace first)");
    h->weights_ready = true;
    return Y4_OK;
}

static int forward_impl(y4_handle h, const void* imgs, bool u8, int n, void* stream) {
    if (int r = check_ready(h, n)) return r;
    Y4_REQUIRE(imgs, Y4_EINVAL, "y4_forward: null images");
    h->img_u8 = u8;
    std::vector<Launch> sched;
    build_schedule(h, n, sched);
    int rc = Y4_OK;
    for (const Launch& l : sched)
        if ((rc = run_op(h, l.op, imgs, l.cnt, (hipStream_t)stream, l.img0))) break;
    h->img_u8 = false;
    return rc;
}

// The forward pass up to and including conv `last_conv` (bench.py's backbone-only mode: last_conv = 71 is CSPDarknet53 proper,
// reference custom_layers.py:100-124).  The conv must end a launch: a run / residual-block kernel that is in force and continues
// past it is refused instead of being cut.
int y4_forward_until(y4_handle h, const float* imgs, int n, int last_conv, void* stream) {
    if (int r = check_ready(h, n)) return r;
    Y4_REQUIRE(imgs, Y4_EINVAL, "y4_forward_until: null images");
    int last_op = -1;
    for (int i = 0; i < (int)h->ops.size(); ++i)
        if (h->ops[i].kind != OP_SPP && (h->ops[i].conv == last_conv || h->ops[i].conv2 == last_conv)) last_op = i;
    Y4_REQUIRE(last_op >= 0, Y4_EINVAL, "y4_forward_until: no conv %d", last_conv);
    for (const Chain& ch : h->chains)
        Y4_REQUIRE(!(h->chain_active(ch) && ch.head <= last_op && (ch.tail[0] > last_op || ch.tail[1] > last_op)), Y4_EINVAL,
                   "y4_forward_until: conv %d sits inside a fused run that continues behind it", last_conv);
    Y4_REQUIRE(!h->heads_res(last_op), Y4_EINVAL, "y4_forward_until: conv %d heads a residual-block kernel that continues behind it", last_conv);
    Y4_REQUIRE(!(h->stage_active() && last_op >= h->stage_first && last_op < h->stage_last), Y4_EINVAL,
               "y4_forward_until: conv %d sits inside the stage kernel", last_conv);
    Y4_REQUIRE(!(h->sched.fuse_stem && last_op == 0), Y4_EINVAL, "y4_forward_until: conv 0 runs fused with conv 1");
    h->img_u8 = false;
    std::vector<Launch> sched;
    build_schedule(h, n, sched);
    int rc = Y4_OK;
    for (const Launch& l : sched)
        if (l.op <= last_op && (rc = run_op(h, l.op, imgs, l.cnt, (hipStream_t)stream, l.img0))) break;
    return rc;
}

int y4_forward(y4_handle h, const float* imgs, int n, void* stream) { return forward_impl(h, imgs, false, n, stream); }
int y4_forward_u8(y4_handle h, const uint8_t* imgs, int n, void* stream) { return forward_impl(h, imgs, true, n, stream); }

int y4_get_heads(y4_handle h, int n, float* out_s, float* out_m, float* out_l, void* stream) {
    if (int r = check_ready(h, n)) return r;
    float* outs[3] = {out_s, out_m, out_l};
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        const View& v = h->heads[i];
        if (int r = view_to_f32_launch(Y4_F32, buf_ptr(h, v), outs[i], (int64_t)n * v.h * v.w, v.cstride, v.coff,
                                       v.c, (hipStream_t)stream))
            return r;
    }
    return Y4_OK;
}

int y4_set_heads(y4_handle h, int n, const float* in_s, const float* in_m, const float* in_l, void* stream) {
    if (int r = check_ready(h, n)) return r;
    const float* ins[3] = {in_s, in_m, in_l};
    for (int i = 0; i < 3; ++i) {
        Y4_REQUIRE(ins[i], Y4_EINVAL, "y4_set_heads: null head %d", i);
        h->obj_n[i] = -1;
        const View& v = h->heads[i];
        if (int r = f32_to_view_launch(ins[i], (float*)buf_ptr(h, v), (int64_t)n * v.h * v.w, v.cstride, v.c,
                                       (hipStream_t)stream))
            return r;
    }
    return Y4_OK;
}

int y4_get_conv_output(y4_handle h, int conv_idx, int n, float* out, size_t out_floats, void* stream) {
    if (int r = check_ready(h, n)) return r;
    Y4_REQUIRE(!h->alias_bufs, Y4_ESTATE, "intermediate tensors are not retained with workspace aliasing on");
    for (const Op& op : h->ops) {
        if (op.kind == OP_SPP || (op.conv != conv_idx && op.conv2 != conv_idx)) continue;
        Y4_REQUIRE(!(h->sched.fuse_stem && conv_idx == 0), Y4_ESTATE, "conv 0 is not materialised while stem fusion is on");
        const int oi = (int)(&op - h->ops.data());
        Y4_REQUIRE(!(h->stage_active() && oi >= h->stage_first && oi < h->stage_last), Y4_ESTATE,
                   "conv %d is not materialised while the stage fusion is on", conv_idx);
        Y4_REQUIRE(!h->heads_res(oi), Y4_ESTATE, "conv %d is not materialised while the residual-block fusion is on", conv_idx);
        const View& v = op.conv == conv_idx ? op.out : op.out2;
        const int64_t px = (int64_t)n * v.h * v.w;   // for an upsampling conv: the upsampled tensor
        Y4_REQUIRE((int64_t)out_floats >= px * v.c, Y4_EINVAL, "output buffer too small: %zu < %lld", out_floats,
                   (long long)(px * v.c));
        return view_to_f32_launch(op.out_f32 ? Y4_F32 : h->cfg.dtype, buf_ptr(h, v), out, px, v.cstride, v.coff, v.c,
                                  (hipStream_t)stream);
    }
    set_error("no conv with index %d", conv_idx);
    return Y4_EINVAL;
}

int y4_decode_nms(y4_handle h, int n, float iou_threshold, float score_threshold, float* boxes, float* scores,
                  float* classes, int32_t* valid, int32_t* kept_idx, void* stream) {
    return y4_decode_nms_mapped(h, n, iou_threshold, score_threshold, nullptr, boxes, scores, classes, valid, kept_idx, stream);
}

int y4_decode_nms_mapped(y4_handle h, int n, float iou_threshold, float score_threshold, const float* box_map, float* boxes,
                         float* scores, float* classes, int32_t* valid, int32_t* kept_idx, void* stream) {
    if (int r = check_ready(h, n)) return r;
    Y4_REQUIRE(boxes && scores && classes && valid, Y4_EINVAL, "y4_decode_nms: null output");
    return detect_tail(h, "y4_decode_nms", nullptr, n, iou_threshold, score_threshold, 0, nullptr, NmsOutputs{boxes, scores, classes, valid, kept_idx},
                       box_map, (hipStream_t)stream);
}

int y4_decode_nms_merged(y4_handle h, int n, float iou_threshold, float score_threshold, const float* box_map, int32_t* cand_count,
                         float* boxes, float* scores, float* classes, int32_t* valid, int32_t* kept_idx, void* stream) {
    if (int r = check_ready(h, n)) return r;
    Y4_REQUIRE(cand_count && boxes && scores && classes && valid && kept_idx, Y4_EINVAL, "y4_decode_nms_merged: null output");
    return detect_tail(h, "y4_decode_nms_merged", nullptr, n, iou_threshold, score_threshold, TAIL_COUNTS | TAIL_MERGE, cand_count,
                       NmsOutputs{boxes, scores, classes, valid, kept_idx}, box_map, (hipStream_t)stream);
}

int y4_set_nms_rule(y4_handle h, int kind, float beta, int agnostic) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(kind == 0 || kind == 1, Y4_EINVAL, "y4_set_nms_rule: kind %d (0: IoU, 1: DIoU)", kind);
    Y4_REQUIRE(std::isfinite(beta) && beta > 0.f, Y4_EINVAL, "y4_set_nms_rule: beta %g must be finite and > 0", (double)beta);
    Y4_REQUIRE(agnostic == 0 || agnostic == 1, Y4_EINVAL, "y4_set_nms_rule: agnostic %d (0 or 1)", agnostic);
    h->nms_kind = kind; h->nms_beta = beta; h->nms_agnostic = agnostic;
    return Y4_OK;
}

int y4_get_nms_rule(y4_handle h, int* kind, float* beta, int* agnostic) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(kind && beta && agnostic, Y4_EINVAL, "y4_get_nms_rule: null argument");
    *kind = h->nms_kind; *beta = h->nms_beta; *agnostic = h->nms_agnostic;
    return Y4_OK;
}

// The two score-decay modes of the NMS stage: what y4_set_nms_soft and y4_set_nms_matrix differ in
struct Decay {
    const char* name;                  // y4_set_<name>, y4_get_<name>: for messages
    int max_method;
    const char* methods;               // ... spelled out
    DecayMode y4_ctx::*own;
    DecayMode y4_ctx::*other;          // the mode that must be off while this one is on
    const char* other_name;
};
static const Decay SOFT{"nms_soft", 3, "0: off, 1: gaussian, 2: linear, 3: hard", &y4_ctx::soft, &y4_ctx::matrix,
                        "Matrix-NMS is on (y4_set_nms_matrix)"};
static const Decay MATRIX{"nms_matrix", 2, "0: off, 1: gaussian, 2: linear", &y4_ctx::matrix, &y4_ctx::soft,
                          "Soft-NMS is on (y4_set_nms_soft)"};

static int set_decay(y4_handle h, const Decay& d, int method, float sigma, float min_score, int top_k) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(method >= 0 && method <= d.max_method, Y4_EINVAL, "y4_set_%s: method %d (%s)", d.name, method, d.methods);
    Y4_REQUIRE(std::isfinite(sigma) && sigma > 0.f, Y4_EINVAL, "y4_set_%s: sigma %g must be finite and > 0", d.name, (double)sigma);
    Y4_REQUIRE(std::isfinite(min_score) && min_score < 1.f, Y4_EINVAL, "y4_set_%s: min_score %g must be finite and < 1", d.name, (double)min_score);
    Y4_REQUIRE(top_k >= 1 && top_k <= 4096, Y4_EINVAL, "y4_set_%s: top_k %d outside 1 .. 4096", d.name, top_k);
    Y4_REQUIRE(method == 0 || (h->*d.other).method == 0, Y4_EINVAL, "y4_set_%s: method %d while %s", d.name, method, d.other_name);
    h->*d.own = DecayMode{method, sigma, min_score, top_k};
    return Y4_OK;
}

static int get_decay(y4_handle h, const Decay& d, int* method, float* sigma, float* min_score, int* top_k) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(method && sigma && min_score && top_k, Y4_EINVAL, "y4_get_%s: null argument", d.name);
    const DecayMode& m = h->*d.own;
    *method = m.method; *sigma = m.sigma; *min_score = m.min_score; *top_k = m.top_k;
    return Y4_OK;
}

int y4_set_nms_soft(y4_handle h, int method, float sigma, float min_score, int top_k) { return set_decay(h, SOFT, method, sigma, min_score, top_k); }
int y4_get_nms_soft(y4_handle h, int* method, float* sigma, float* min_score, int* top_k) { return get_decay(h, SOFT, method, sigma, min_score, top_k); }
int y4_set_nms_matrix(y4_handle h, int method, float sigma, float min_score, int top_k) { return set_decay(h, MATRIX, method, sigma, min_score, top_k); }
int y4_get_nms_matrix(y4_handle h, int* method, float* sigma, float* min_score, int* top_k) { return get_decay(h, MATRIX, method, sigma, min_score, top_k); }

// ---- gathered decode + NMS (tiled inference).  The caller's scratch: [n_groups] counters, one per 256-byte line | the groups' key
// lists [n_groups][group_cap] | the groups' box tables [n_groups][max_slots * nbox][4], each part 256-byte aligned.
struct GatherLayout { size_t keys_off, boxes_off, bytes; };
static int gather_layout(y4_handle h, const char* who, int n_groups, int max_slots, uint32_t group_cap, GatherLayout* L) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(n_groups >= 1 && max_slots >= 1 && group_cap >= 1, Y4_EINVAL, "%s: n_groups %d, max_slots %d, group_cap %u (all >= 1)", who,
               n_groups, max_slots, group_cap);
    Y4_REQUIRE((int64_t)max_slots * h->nbox * h->cfg.num_classes < (1ll << 31), Y4_EINVAL,
               "%s: %d slots of %d boxes and %d classes exceed the 2^31 candidate ids a key holds", who, max_slots, h->nbox,
               h->cfg.num_classes);
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    L->keys_off = up((size_t)n_groups * COUNT_STRIDE * sizeof(uint32_t));
    L->boxes_off = L->keys_off + up((size_t)n_groups * group_cap * 8);
    L->bytes = L->boxes_off + up((size_t)n_groups * max_slots * h->nbox * 16);
    return Y4_OK;
}
// the groups' lists in the scratch as a candidate store: a group's box table is max_slots rows' boxes
static CandStore gathered_cands(y4_handle h, void* scratch, const GatherLayout& L, int max_slots, uint32_t group_cap) {
    char* sp = (char*)scratch;
    return cand_store(h, (float*)(sp + L.boxes_off), (unsigned long long*)(sp + L.keys_off), (uint32_t*)sp, group_cap, max_slots * h->nbox);
}
static int gather_scratch_check(const char* who, const void* scratch) {
    Y4_REQUIRE(scratch, Y4_EINVAL, "%s: null scratch", who);
    Y4_REQUIRE(((uintptr_t)scratch & 255) == 0, Y4_EINVAL, "%s: scratch must be 256-byte aligned", who);
    return Y4_OK;
}

int y4_gather_scratch_bytes(y4_handle h, int n_groups, int max_slots, uint32_t group_cap, size_t* bytes) {
    GatherLayout L;
    if (int r = gather_layout(h, "y4_gather_scratch_bytes", n_groups, max_slots, group_cap, &L)) return r;
    Y4_REQUIRE(bytes, Y4_EINVAL, "y4_gather_scratch_bytes: null argument");
    *bytes = L.bytes;
    return Y4_OK;
}

int y4_gather_begin(y4_handle h, int n_groups, int max_slots, uint32_t group_cap, void* scratch_dev, void* stream) {
    GatherLayout L;
    if (int r = gather_layout(h, "y4_gather_begin", n_groups, max_slots, group_cap, &L)) return r;
    if (int r = gather_scratch_check("y4_gather_begin", scratch_dev)) return r;
    Y4_CHECK_HIP(hipMemsetAsync(scratch_dev, 0, (size_t)n_groups * COUNT_STRIDE * sizeof(uint32_t), (hipStream_t)stream));
    return Y4_OK;
}

static int decode_gather(y4_handle h, const char* who, bool oriented, int n, float score_threshold, const int32_t* row_group_dev,
                         const int32_t* row_slot_dev, const float* row_map_dev, int n_groups, int max_slots, uint32_t group_cap,
                         void* scratch_dev, void* stream) {
    GatherLayout L;
    if (int r = gather_layout(h, who, n_groups, max_slots, group_cap, &L)) return r;
    if (int r = check_ready(h, n)) return r;
    if (int r = gather_scratch_check(who, scratch_dev)) return r;
    Y4_REQUIRE(row_group_dev && row_slot_dev && row_map_dev, Y4_EINVAL, "%s: null row table", who);
    const float sc = score_threshold < 0.f ? h->cfg.score_threshold : score_threshold;
    hipStream_t s = (hipStream_t)stream;
    if (int r = run_decode(h, n, sc, s)) return r;
    const CandStore c = workspace_cands(h), g = gathered_cands(h, scratch_dev, L, max_slots, group_cap);
    GatherK k{};
    k.dboxes = c.dboxes; k.keys = c.keys; k.counts = c.counts; k.cap = c.cap;
    k.C = h->cfg.num_classes; k.nbox = c.nbox;
    k.row_group = row_group_dev; k.row_slot = row_slot_dev; k.row_map = row_map_dev;
    k.n_groups = n_groups; k.max_slots = max_slots; k.group_cap = g.cap;
    k.gcounts = g.counts; k.gkeys = g.keys; k.gboxes = g.dboxes;
    k.status = c.status; k.div_c = c.div_c;
    if (int r = gather_launch(k, n, oriented, s)) return r;
    // gather_kernel left the counters of rows 0 .. n-1 at zero, the rows this decode counted into: the handle is where an NMS over
    // n images would have left it (run_nms: counts_clean = counts_n <= n)
    h->counts_clean = true;
    return Y4_OK;
}

int y4_decode_gather(y4_handle h, int n, float score_threshold, const int32_t* row_group_dev, const int32_t* row_slot_dev,
                     const float* row_map_dev, int n_groups, int max_slots, uint32_t group_cap, void* scratch_dev, void* stream) {
    return decode_gather(h, "y4_decode_gather", false, n, score_threshold, row_group_dev, row_slot_dev, row_map_dev, n_groups,
                         max_slots, group_cap, scratch_dev, stream);
}

int y4_decode_gather_views(y4_handle h, int n, float score_threshold, const int32_t* row_group_dev, const int32_t* row_slot_dev,
                           const float* row_map_dev, int n_groups, int max_slots, uint32_t group_cap, void* scratch_dev,
                           void* stream) {
    return decode_gather(h, "y4_decode_gather_views", true, n, score_threshold, row_group_dev, row_slot_dev, row_map_dev, n_groups,
                         max_slots, group_cap, scratch_dev, stream);
}

int y4_nms_gathered(y4_handle h, int n_groups, int max_slots, uint32_t group_cap, float iou_threshold, void* scratch_dev,
                    int32_t* cand_count_dev, float* boxes_dev, float* scores_dev, float* classes_dev, int32_t* valid_dev,
                    int32_t* kept_idx_dev, void* stream) {
    GatherLayout L;
    if (int r = gather_layout(h, "y4_nms_gathered", n_groups, max_slots, group_cap, &L)) return r;
    if (int r = gather_scratch_check("y4_nms_gathered", scratch_dev)) return r;
    Y4_REQUIRE(h->act, Y4_ESTATE, "workspace not bound (call y4_bind_workspace first)");
    Y4_REQUIRE(cand_count_dev && boxes_dev && scores_dev && classes_dev && valid_dev, Y4_EINVAL, "y4_nms_gathered: null output");
    const CandStore g = gathered_cands(h, scratch_dev, L, max_slots, group_cap);
    return detect_tail(h, "y4_nms_gathered", &g, n_groups, iou_threshold, -1.f, TAIL_COUNTS, cand_count_dev,
                       NmsOutputs{boxes_dev, scores_dev, classes_dev, valid_dev, kept_idx_dev}, nullptr, (hipStream_t)stream);
}

int y4_nms_gathered_merged(y4_handle h, int n_groups, int max_slots, uint32_t group_cap, float iou_threshold, void* scratch_dev,
                           int32_t* cand_count_dev, float* boxes_dev, float* scores_dev, float* classes_dev, int32_t* valid_dev,
                           int32_t* kept_idx_dev, void* stream) {
    GatherLayout L;
    if (int r = gather_layout(h, "y4_nms_gathered_merged", n_groups, max_slots, group_cap, &L)) return r;
    if (int r = gather_scratch_check("y4_nms_gathered_merged", scratch_dev)) return r;
    Y4_REQUIRE(h->act, Y4_ESTATE, "workspace not bound (call y4_bind_workspace first)");
    Y4_REQUIRE(cand_count_dev && boxes_dev && scores_dev && classes_dev && valid_dev && kept_idx_dev, Y4_EINVAL,
               "y4_nms_gathered_merged: null output");
    const CandStore g = gathered_cands(h, scratch_dev, L, max_slots, group_cap);
    return detect_tail(h, "y4_nms_gathered_merged", &g, n_groups, iou_threshold, -1.f, TAIL_COUNTS | TAIL_MERGE, cand_count_dev,
                       NmsOutputs{boxes_dev, scores_dev, classes_dev, valid_dev, kept_idx_dev}, nullptr, (hipStream_t)stream);
}

static void loss_geometry(y4_handle h, int* gh, int* gw, int* lane_base) {
    int lanes = 0;
    for (int i = 0; i < 3; ++i) {
        gh[i] = h->heads[i].h; gw[i] = h->heads[i].w;
        if (lane_base) lane_base[i] = lanes;
        lanes += 3 * gh[i] * gw[i];
    }
}

int y4_loss_assign(y4_handle h, int n, const float* boxes, int max_boxes, float* xywh, int32_t* records, int32_t* counts,
                   void* stream) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(n >= 1, Y4_EINVAL, "y4_loss_assign: batch %d", n);
    Y4_REQUIRE(boxes && xywh && records && counts, Y4_EINVAL, "y4_loss_assign: null argument");
    LossAssignK k{};
    k.boxes = boxes; k.xywh = xywh; k.records = records; k.counts = counts;
    k.mb = max_boxes; k.C = h->cfg.num_classes; k.mw = (k.C + 31) / 32; k.rw = 8 + k.mw;
    k.img_h = h->H; k.img_w = h->W;
    loss_geometry(h, k.gh, k.gw, k.lane_base);
    memcpy(k.anchors, h->cfg.anchors, sizeof(k.anchors));
    return loss_assign_launch(k, n, (hipStream_t)stream);
}

int y4_loss_scratch_floats(y4_handle h, int n, size_t* floats) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(n >= 1 && floats, Y4_EINVAL, "y4_loss_scratch_floats: bad argument");
    int gh[3], gw[3];
    loss_geometry(h, gh, gw, nullptr);
    *floats = (size_t)n * loss_strips(gh, gw, nullptr) * 3;
    return Y4_OK;
}

// what y4_loss and the three gradient entry points share: the heads, the loss geometry and one batch's labels
static void loss_inputs(y4_handle h, LossIn& k, const int32_t* records, const int32_t* counts, const float* xywh, int max_boxes,
                        float iou_loss_thresh, const float* img_weight) {
    loss_geometry(h, k.gh, k.gw, nullptr);
    k.strips = loss_strips(k.gh, k.gw, k.strip_base);
    for (int i = 0; i < 3; ++i) {
        k.head[i] = (const float*)buf_ptr(h, h->heads[i]);
        k.stride[i] = (float)h->cfg.strides[i];
    }
    memcpy(k.anchors, h->cfg.anchors, sizeof(k.anchors));
    k.C = h->cfg.num_classes; k.hcs = h->hcs; k.mb = max_boxes; k.rw = 8 + (k.C + 31) / 32;
    k.thresh = iou_loss_thresh;
    k.input_area = (float)h->H * (float)h->W;          // input_size ** 2 of the reference (loss.py:158); H * W for a rectangle
    k.records = records; k.counts = counts; k.xywh = xywh; k.imgw = img_weight;
    k.box_kind = h->box_kind;
}

int y4_set_box_loss(y4_handle h, int kind) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(kind == BOX_GIOU || kind == BOX_CIOU, Y4_EINVAL, "y4_set_box_loss: kind %d (0: GIoU, 1: CIoU)", kind);
    h->box_kind = kind;
    return Y4_OK;
}

int y4_get_box_loss(y4_handle h) {
    if (int r = check_handle(h)) return r;
    return h->box_kind;
}

int y4_loss(y4_handle h, int n, const int32_t* records, const int32_t* counts, const float* xywh, int max_boxes,
            float iou_loss_thresh, float* scratch, size_t scratch_floats, float* out, void* stream) {
    if (int r = check_ready(h, n)) return r;
    Y4_REQUIRE(records && counts && xywh && scratch && out, Y4_EINVAL, "y4_loss: null argument");
    Y4_REQUIRE(iou_loss_thresh >= 0.f, Y4_EINVAL, "y4_loss: iou_loss_thresh %g", (double)iou_loss_thresh);
    LossK k{};
    loss_inputs(h, k, records, counts, xywh, max_boxes, iou_loss_thresh, nullptr);
    Y4_REQUIRE(scratch_floats >= (size_t)n * k.strips * 3, Y4_ENOMEM, "y4_loss: scratch %zu < %zu floats", scratch_floats,
               (size_t)n * k.strips * 3);
    k.partials = scratch; k.out = out;
    return loss_launch(k, n, (hipStream_t)stream);
}

// ---- head fine-tuning (head_train.hip)

// the op of head conv `i` (93 / 101 / 109)
static const Op* head_op(y4_handle h, int i) {
    for (const Op& o : h->ops)
        if (o.out_f32 && o.out.buf == h->heads[i].buf) return &o;
    return nullptr;
}
// the op of the conv in front of it (92 / 100 / 108): the one that writes the head conv's input
static const Op* block_op(y4_handle h, int i) {
    const Op* ho = head_op(h, i);
    if (!ho) return nullptr;
    for (const Op& o : h->ops)
        if (o.kind == OP_CONV && same_view(o.out, ho->in)) return &o;
    return nullptr;
}

int y4_set_retain_head_inputs(y4_handle h, int on) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(!h->act, Y4_ESTATE, "y4_set_retain_head_inputs: the workspace is already bound (call it before y4_workspace_bytes / y4_bind_workspace)");
    // level 2 relies on the plan, not on a switch: a run keeps only its head's output on chip, its tail is a 1x1 conv, and the
    // inputs of convs 92 / 100 / 108 are each the output of a 1x1 conv that is the tail of its run or has a reader outside it
    if (on == 2)
        for (const Chain& ch : h->chains)
            for (int i = 0; i < 3; ++i)
                if (const Op* b = block_op(h, i))
                    Y4_REQUIRE(h->ops[ch.head].out.buf != b->in.buf || h->stores_x(ch), Y4_ESTATE,
                               "y4_set_retain_head_inputs: a fused run keeps the input of conv %d on chip", h->layers[b->conv].d.idx);
    h->retain_head_in = on != 0;                                         // (every non-zero value but 2 is level 1, as before level 2 existed)
    h->retain_block_in = on == 2;                                        // (y4_ctx::stores_x: the LDS pairs in front of the heads follow)
    layout(*h);
    return Y4_OK;
}

// A trainable group: three convs, one per scale, whose float32 records lie back to back in the gradient, master-weight and
// moment buffers.  A record is [cout biases, if the group trains them][cout x cin x ksize x ksize weights].  (The fragment-order
// copy of a 3x3 conv's weights needs no column: Layer::has_frag says where one exists, and no 1x1 conv has one.)
struct Group {
    const Op* (*op)(y4_handle, int);   // the group's conv of scale i
    int ksize;
    bool bias;                         // the record opens with the biases, which reach the packed weights through fold_bn_launch
    const char *noun, *unit, *grad;    // for messages
};
static const Group HEADS{head_op, 1, true, "three head records", "head", "dw"};
static const Group BLOCKS{block_op, 3, false, "three kernels", "scale", "dk"};

// float offsets of the group's three records and their total
static size_t group_offsets(y4_handle h, const Group& g, size_t* off) {
    size_t total = 0;
    for (int i = 0; i < 3; ++i) {
        const Layer& L = h->layers[g.op(h, i)->conv];
        if (off) off[i] = total;
        total += (size_t)L.d.cout * ((g.bias ? 1 : 0) + (size_t)L.d.cin * g.ksize * g.ksize);
    }
    return total;
}

// the channels of the group's three convs
static void group_channels(y4_handle h, const Group& g, int* cin, int* cout) {
    for (int i = 0; i < 3; ++i) {
        const Layer& L = h->layers[g.op(h, i)->conv];
        cin[i] = L.d.cin;
        if (cout) cout[i] = L.d.cout;
    }
}

// the shared front of y4_head_grad / y4_block_grad: the arguments, the labels into k, dense inputs, the size of dw -> offsets
static int grad_front(y4_handle h, const Group& g, const char* who, GradK& k, const int32_t* records, const int32_t* counts,
                      const float* xywh, int max_boxes, float iou_loss_thresh, const float* img_weight, const void* scratch,
                      const float* dw, size_t dw_floats, size_t* off) {
    Y4_REQUIRE(records && counts && xywh && img_weight && scratch && dw, Y4_EINVAL, "%s: null argument", who);
    Y4_REQUIRE(iou_loss_thresh >= 0.f, Y4_EINVAL, "%s: iou_loss_thresh %g", who, (double)iou_loss_thresh);
    loss_inputs(h, k, records, counts, xywh, max_boxes, iou_loss_thresh, img_weight);
    for (int i = 0; i < 3; ++i)
        for (const View& v : {head_op(h, i)->in, g.op(h, i)->in})
            Y4_REQUIRE(v.coff == 0 && v.cstride == v.c, Y4_EINVAL, "%s: %s %d reads a channel slice", who, g.unit, i);
    const size_t total = group_offsets(h, g, off);
    Y4_REQUIRE(dw_floats >= total, Y4_ENOMEM, "%s: %s %zu < %zu floats", who, g.grad, dw_floats, total);
    return Y4_OK;
}

// Adam on the group's master weights and the re-pack: what y4_pack_weights does with these three records (same kernels, same
// rounding), every packed copy.  A group without biases leaves scale / shift alone: its BatchNormalization is frozen, so what
// fold_bn made of it at y4_pack_weights is already what a fresh load makes.
static int adam_step(y4_handle h, const Group& g, const char* who, const float* dw, float* w, float* m, float* v, size_t n_floats,
                     float lr, float beta1, float beta2, float epsilon, int t, void* stream) {
    Y4_REQUIRE(dw && w && m && v, Y4_EINVAL, "%s: null argument", who);
    Y4_REQUIRE(t >= 1, Y4_EINVAL, "%s: step %d (the first step is 1)", who, t);
    size_t off[3];
    const size_t total = group_offsets(h, g, off);
    Y4_REQUIRE(n_floats == total, Y4_EINVAL, "%s: %zu floats, the %s have %zu", who, n_floats, g.noun, total);
    hipStream_t s = (hipStream_t)stream;
    const float lr_t = (float)((double)lr * sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t)));
    if (int r = adam_launch(dw, w, m, v, total, lr_t, beta1, beta2, epsilon, s)) return r;
    for (int i = 0; i < 3; ++i) {
        const Layer& L = h->layers[g.op(h, i)->conv];
        const float* rec = w + off[i];
        if (g.bias)
            if (int r = fold_bn_launch(rec, (float*)(h->wts + L.scale_off), (float*)(h->wts + L.shift_off), L.d.cout, L.cout_pad, 0, s))
                return r;
        if (int r = pack_conv_weights(h->cfg.dtype, L.d.cout, L.d.cin, g.ksize, rec + (g.bias ? L.d.cout : 0), h->wts + L.w_off, s)) return r;
        if (L.has_frag)
            if (int r = pack_conv_frag32(h->cfg.dtype, L.d.cout, L.d.cin, h->wts + L.w_off, h->wts + L.frag_off, s)) return r;
    }
    return Y4_OK;
}

static int check_packed(y4_handle h, const char* who) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(h->act && h->wts && h->weights_ready, Y4_ESTATE, "%s: weights not packed (call y4_pack_weights first)", who);
    return Y4_OK;
}

int y4_loss_grad(y4_handle h, int n, const int32_t* records, const int32_t* counts, const float* xywh, int max_boxes,
                 float iou_loss_thresh, const float* img_weight, float* out_s, float* out_m, float* out_l, void* stream) {
    if (int r = check_ready(h, n)) return r;
    Y4_REQUIRE(records && counts && xywh && img_weight && out_s && out_m && out_l, Y4_EINVAL, "y4_loss_grad: null argument");
    Y4_REQUIRE(iou_loss_thresh >= 0.f, Y4_EINVAL, "y4_loss_grad: iou_loss_thresh %g", (double)iou_loss_thresh);
    GradK k{};
    loss_inputs(h, k, records, counts, xywh, max_boxes, iou_loss_thresh, img_weight);
    k.dense[0] = out_s; k.dense[1] = out_m; k.dense[2] = out_l;
    return loss_grad_launch(k, n, (hipStream_t)stream);
}

int y4_head_grad_scratch_floats(y4_handle h, int n, size_t* floats) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(n >= 1 && floats, Y4_EINVAL, "y4_head_grad_scratch_floats: bad argument");
    int gh[3], gw[3], cin[3];
    loss_geometry(h, gh, gw, nullptr);
    group_channels(h, HEADS, cin, nullptr);
    *floats = head_grad_scratch_floats(gh, gw, cin, n, nullptr);
    return Y4_OK;
}

int y4_head_grad(y4_handle h, int n, const int32_t* records, const int32_t* counts, const float* xywh, int max_boxes,
                 float iou_loss_thresh, const float* img_weight, float* scratch, size_t scratch_floats, float* dw, size_t dw_floats,
                 int accumulate, void* stream) {
    if (int r = check_ready(h, n)) return r;
    Y4_REQUIRE(h->retain_head_in, Y4_ESTATE, "y4_head_grad: the head convs' inputs are not retained (y4_set_retain_head_inputs before "
               "the workspace is bound)");
    GradK k{};
    if (int r = grad_front(h, HEADS, "y4_head_grad", k, records, counts, xywh, max_boxes, iou_loss_thresh, img_weight, scratch, dw,
                           dw_floats, k.dw_off))
        return r;
    group_channels(h, HEADS, k.cin, nullptr);
    head_grad_strips(k.gh, k.gw, k.pstrip_base, k.pstrips);
    const size_t need = head_grad_scratch_floats(k.gh, k.gw, k.cin, n, k.part_base);
    Y4_REQUIRE(scratch_floats >= need, Y4_ENOMEM, "y4_head_grad: scratch %zu < %zu floats", scratch_floats, need);
    for (int i = 0; i < 3; ++i) k.x[i] = buf_ptr(h, head_op(h, i)->in);
    k.partials = scratch; k.dw = dw; k.accumulate = accumulate != 0;
    return head_grad_launch(h->cfg.dtype, k, n, (hipStream_t)stream);
}

int y4_head_adam(y4_handle h, const float* dw, float* w, float* m, float* v, size_t n_floats, float lr, float beta1, float beta2,
                 float epsilon, int t, void* stream) {
    if (int r = check_packed(h, "y4_head_adam")) return r;
    return adam_step(h, HEADS, "y4_head_adam", dw, w, m, v, n_floats, lr, beta1, beta2, epsilon, t, stream);
}

// ---- fine-tuning of the 3x3 convs in front of the heads (block_train.hip)

static int block_check(y4_handle h, const char* who) {
    for (int i = 0; i < 3; ++i) {
        const Op* b = block_op(h, i);
        Y4_REQUIRE(b != nullptr, Y4_EINVAL, "%s: no conv in front of head %d", who, i);
        const Layer& L = h->layers[b->conv];
        Y4_REQUIRE(L.d.ksize == 3 && L.d.stride == 1 && L.d.act == Y4_ACT_LEAKY && L.d.has_bn && !b->has_res && !b->upsample && b->conv2 < 0 &&
                   L.fused_with < 0 && L.extra_rows == 0, Y4_EINVAL, "%s: conv %d is not a plain 3x3 Conv + BN + LeakyReLU", who, L.d.idx);
    }
    return Y4_OK;
}

int y4_block_grad_scratch_bytes(y4_handle h, int n, size_t* bytes) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(n >= 1 && bytes, Y4_EINVAL, "y4_block_grad_scratch_bytes: bad argument");
    if (int r = block_check(h, "y4_block_grad_scratch_bytes")) return r;
    int gh[3], gw[3], cin[3], cout[3];
    loss_geometry(h, gh, gw, nullptr);
    group_channels(h, BLOCKS, cin, cout);
    *bytes = block_grad_scratch_bytes(h->cfg.dtype, n, gh, gw, cin, cout, nullptr, nullptr);
    Y4_REQUIRE(*bytes > 0, Y4_EINVAL, "y4_block_grad_scratch_bytes: a grid row of %d cells does not fit the weight gradient's LDS tile", gw[0]);
    return Y4_OK;
}

// y4_block_grad (scale 1, no overflow word) and y4_block_grad_scaled
static int block_grad_impl(y4_handle h, const char* who, int n, const int32_t* records, const int32_t* counts, const float* xywh,
                           int max_boxes, float iou_loss_thresh, const float* img_weight, float loss_scale, int32_t* overflow,
                           void* scratch, size_t scratch_bytes, float* dk, size_t dk_floats, int accumulate, void* stream) {
    if (int r = block_check(h, who)) return r;
    Y4_REQUIRE(h->retain_block_in, Y4_ESTATE, "%s: the inputs of convs 92 / 100 / 108 are not retained (retention level 2: "
               "y4_set_retain_head_inputs(h, 2) before the workspace is bound)", who);
    GradK k{};
    BlockK b{};
    if (int r = grad_front(h, BLOCKS, who, k, records, counts, xywh, max_boxes, iou_loss_thresh, img_weight, scratch, dk, dk_floats,
                           b.dk_off))
        return r;
    Y4_REQUIRE(((uintptr_t)scratch & 255) == 0, Y4_EINVAL, "%s: scratch must be 256-byte aligned", who);
    group_channels(h, BLOCKS, b.cin, b.cout);
    block_dgrad_strips(k.gh, k.gw, b.dstrip_base);
    size_t dz_off[3], part_off[3];
    const size_t need = block_grad_scratch_bytes(h->cfg.dtype, n, k.gh, k.gw, b.cin, b.cout, dz_off, part_off);
    Y4_REQUIRE(need > 0, Y4_EINVAL, "%s: a grid row of %d cells does not fit the weight gradient's LDS tile", who, k.gw[0]);
    Y4_REQUIRE(scratch_bytes >= need, Y4_ENOMEM, "%s: scratch %zu < %zu bytes", who, scratch_bytes, need);
    for (int i = 0; i < 3; ++i) {
        const Op* ho = head_op(h, i);
        const Op* bo = block_op(h, i);
        b.u[i] = buf_ptr(h, bo->in); b.a[i] = buf_ptr(h, ho->in);
        b.wh[i] = h->wts + h->layers[ho->conv].w_off; b.bn_scale[i] = (const float*)(h->wts + h->layers[bo->conv].scale_off);
        b.dz[i] = (char*)scratch + dz_off[i]; b.part[i] = (float*)((char*)scratch + part_off[i]);
    }
    b.dk = dk; b.accumulate = accumulate != 0;
    b.loss_scale = loss_scale; b.overflow = overflow;
    return block_grad_launch(h->cfg.dtype, k, b, n, (hipStream_t)stream);
}

int y4_block_grad(y4_handle h, int n, const int32_t* records, const int32_t* counts, const float* xywh, int max_boxes,
                  float iou_loss_thresh, const float* img_weight, void* scratch, size_t scratch_bytes, float* dk, size_t dk_floats,
                  int accumulate, void* stream) {
    if (int r = check_ready(h, n)) return r;
    Y4_REQUIRE(h->cfg.dtype != Y4_F16, Y4_EINVAL, "y4_block_grad: an f16 handle needs a loss scale (a 16-bit dZ in fp16 underflows "
               "without one): call y4_block_grad_scaled");
    return block_grad_impl(h, "y4_block_grad", n, records, counts, xywh, max_boxes, iou_loss_thresh, img_weight, 1.0f, nullptr, scratch,
                           scratch_bytes, dk, dk_floats, accumulate, stream);
}

int y4_block_grad_scaled(y4_handle h, int n, const int32_t* records, const int32_t* counts, const float* xywh, int max_boxes,
                         float iou_loss_thresh, const float* img_weight, float loss_scale, int32_t* overflow, void* scratch,
                         size_t scratch_bytes, float* dk, size_t dk_floats, int accumulate, void* stream) {
    if (int r = check_ready(h, n)) return r;
    Y4_REQUIRE(overflow || h->cfg.dtype != Y4_F16, Y4_EINVAL, "y4_block_grad_scaled: an f16 handle needs the overflow word");
    return block_grad_impl(h, "y4_block_grad_scaled", n, records, counts, xywh, max_boxes, iou_loss_thresh, img_weight, loss_scale,
                           overflow, scratch, scratch_bytes, dk, dk_floats, accumulate, stream);
}

int y4_block_adam(y4_handle h, const float* dk, float* w, float* m, float* v, size_t n_floats, float lr, float beta1, float beta2,
                  float epsilon, int t, void* stream) {
    if (int r = check_packed(h, "y4_block_adam")) return r;
    if (int r = block_check(h, "y4_block_adam")) return r;
    return adam_step(h, BLOCKS, "y4_block_adam", dk, w, m, v, n_floats, lr, beta1, beta2, epsilon, t, stream);
}

// ---- cached frozen features (feature_cache.hip)

// the op whose INPUT view scale i's part of a cache row mirrors: the head conv at level 1, the 3x3 conv in front of it at level 2
static const Op* feature_op(y4_handle h, int i) { return h->retain_block_in ? block_op(h, i) : head_op(h, i); }

// the row layout and, with k, the views' side of a copy
static int feature_layout(y4_handle h, const char* who, FeatureK* k, size_t* row_bytes, size_t* offs) {
    Y4_REQUIRE(h->retain_head_in, Y4_ESTATE, "%s: the handle retains nothing (y4_set_retain_head_inputs before the workspace is bound)", who);
    size_t off = 0, chunks = 0;
    for (int i = 0; i < 3; ++i) {
        const Op* o = feature_op(h, i);
        Y4_REQUIRE(o != nullptr, Y4_EINVAL, "%s: no conv in front of head %d", who, i);
        const View& v = o->in;
        const size_t px_bytes = (size_t)v.c * h->es, bytes = (size_t)v.h * v.w * px_bytes;
        Y4_REQUIRE(px_bytes % 16 == 0 && ((size_t)v.cstride * h->es) % 16 == 0 && ((size_t)v.coff * h->es) % 16 == 0, Y4_EINVAL,
                   "%s: scale %d's view (%d channels at %d of %d) is not made of 16-byte chunks", who, i, v.c, v.coff, v.cstride);
        if (offs) offs[i] = off;
        if (k) {
            const Buffer& b = h->bufs[v.buf];
            k->view[i] = h->act ? buf_ptr(h, v) : nullptr;
            k->img_stride[i] = (uint64_t)b.h * b.w * b.channels * h->es;
            k->pix_stride[i] = (uint32_t)(v.cstride * h->es);
            k->coff[i] = (uint32_t)(v.coff * h->es);
            k->first[i] = (uint32_t)chunks;
            k->off[i] = (uint32_t)off;
            k->cpp[i] = fastdiv_make((uint32_t)(px_bytes / 16));
        }
        chunks += bytes / 16;
        off = align256(off + bytes);
    }
    Y4_REQUIRE(chunks < (1u << 30), Y4_EINVAL, "%s: a row of %zu bytes", who, off);
    if (k) { k->row = fastdiv_make((uint32_t)chunks); k->row_bytes = off; }
    if (row_bytes) *row_bytes = off;
    return Y4_OK;
}

int y4_feature_row_bytes(y4_handle h, size_t* row_bytes, size_t offs[3]) {
    if (int r = check_handle(h)) return r;
    return feature_layout(h, "y4_feature_row_bytes", nullptr, row_bytes, offs);
}

// y4_feature_store / y4_feature_load: every refusal first, then one launch per FEATURE_MAX_IMAGES images and 2^31 chunks
static int feature_copy(y4_handle h, const char* who, bool store, int n, const int64_t* slots, void* cache, size_t cache_rows, void* stream) {
    if (int r = check_handle(h)) return r;
    FeatureK k{};
    if (int r = feature_layout(h, who, &k, nullptr, nullptr)) return r;
    Y4_REQUIRE(h->act, Y4_ESTATE, "%s: workspace not bound (call y4_bind_workspace first)", who);
    Y4_REQUIRE(n >= 1 && n <= h->cfg.max_batch, Y4_EINVAL, "%s: batch %d outside [1, max_batch=%d]", who, n, h->cfg.max_batch);
    Y4_REQUIRE(slots && cache, Y4_EINVAL, "%s: null argument", who);
    Y4_REQUIRE(((uintptr_t)cache & 15) == 0, Y4_EINVAL, "%s: the cache must be 16-byte aligned", who);
    for (int i = 0; i < 3; ++i) Y4_REQUIRE(((uintptr_t)k.view[i] & 15) == 0, Y4_EINVAL, "%s: the workspace is not 16-byte aligned", who);
    const int64_t rows = (int64_t)std::min<size_t>(cache_rows, (size_t)INT32_MAX);
    for (int i = 0; i < n; ++i)
        Y4_REQUIRE(slots[i] >= 0 && slots[i] < rows, Y4_EINVAL, "%s: slot %lld of image %d outside [0, %lld)", who, (long long)slots[i], i,
                   (long long)rows);
    if (store) {
        std::vector<int64_t> seen(slots, slots + n);
        std::sort(seen.begin(), seen.end());
        const auto dup = std::adjacent_find(seen.begin(), seen.end());
        Y4_REQUIRE(dup == seen.end(), Y4_EINVAL, "%s: slot %lld is named twice", who, dup == seen.end() ? 0ll : (long long)*dup);
    }
    k.cache = (char*)cache;
    const int per_launch = (int)std::min<uint32_t>(FEATURE_MAX_IMAGES, ((1u << 31) - 1) / k.row.d);
    for (int i0 = 0; i0 < n; i0 += per_launch) {
        const int cnt = std::min(per_launch, n - i0);
        FeatureK g = k;
        for (int i = 0; i < 3; ++i) g.view[i] += (uint64_t)i0 * g.img_stride[i];
        for (int i = 0; i < cnt; ++i) g.slot[i] = (int32_t)slots[i0 + i];
        g.total = (uint32_t)cnt * g.row.d;
        if (int r = feature_copy_launch(g, store, (hipStream_t)stream)) return r;
    }
    return Y4_OK;
}

int y4_feature_store(y4_handle h, int n, const int64_t* slots_host, void* cache_dev, size_t cache_rows, void* stream) {
    return feature_copy(h, "y4_feature_store", true, n, slots_host, cache_dev, cache_rows, stream);
}
int y4_feature_load(y4_handle h, int n, const int64_t* slots_host, const void* cache_dev, size_t cache_rows, void* stream) {
    return feature_copy(h, "y4_feature_load", false, n, slots_host, (void*)cache_dev, cache_rows, stream);
}

int y4_forward_tail(y4_handle h, int n, void* stream) {
    if (int r = check_ready(h, n)) return r;
    Y4_REQUIRE(h->retain_head_in, Y4_ESTATE, "y4_forward_tail: the handle retains nothing (y4_set_retain_head_inputs before the workspace is bound)");
    std::vector<int> tail;                               // the ops behind the cached tensors, in plan order
    for (int i = 0; i < 3; ++i) {
        const Op* ho = head_op(h, i);
        const Op* bo = h->retain_block_in ? block_op(h, i) : nullptr;
        Y4_REQUIRE(ho && (bo || !h->retain_block_in), Y4_EINVAL, "y4_forward_tail: no conv in front of head %d", i);
        tail.push_back((int)(ho - h->ops.data()));
        if (bo) tail.push_back((int)(bo - h->ops.data()));
    }
    std::sort(tail.begin(), tail.end());
    auto in_tail = [&](int oi) { return oi < 0 || std::find(tail.begin(), tail.end(), oi) != tail.end(); };
    // a run executes as one kernel here only when it lies wholly inside the tail; any other fusion would run convs in front of it
    auto fused_here = [&](const Chain& ch) { return h->chain_active(ch) && in_tail(ch.head) && in_tail(ch.tail[0]) && in_tail(ch.tail[1]); };
    for (int oi : tail) {
        const OpExec ex = resolve_op(h, oi, true);
        bool ran_with_head = false;
        if (ex.kind == EX_SKIP)
            for (const Chain& ch : h->chains) ran_with_head |= (ch.tail[0] == oi || ch.tail[1] == oi) && fused_here(ch);
        if (ran_with_head) continue;
        if (int r = run_op(h, oi, nullptr, n, (hipStream_t)stream, 0, ex.chain != nullptr && fused_here(*ex.chain))) return r;
    }
    return Y4_OK;
}

// forward + decode + NMS; when `ev` is given, ev[0] is recorded before the first op and ev[i+1] after op i
static int predict_impl(y4_handle h, const void* imgs, int n, float* boxes, float* scores, float* classes,
                        int32_t* valid, int32_t* kept_idx, hipStream_t s, hipEvent_t* ev) {
    if (int r = check_ready(h, n)) return r;
    Y4_REQUIRE(imgs && boxes && scores && classes && valid, Y4_EINVAL, "y4_predict: null argument");
    std::vector<Launch> sched;
    build_schedule(h, n, sched);
    if (ev && (int)sched.size() + 3 > h->t_per_step) ev = nullptr;       // cannot happen: sized for max_batch
    if (ev && h->t_steps == 0) {
        h->t_n = n;
        h->t_slot_op.clear();
        h->t_rec.assign(sched.size(), 1);
        int seg_first = sched.empty() ? 0 : sched[0].op;
        for (size_t k = 0; k < sched.size(); ++k) {
            const bool last = k + 1 == sched.size();
            // coarse segments: runs of same-kind ops, and the conv family additionally cut behind conv 71 -- the end of
            // CSPDarknet53 proper (reference custom_layers.py:124; north_star words its target on that backbone)
            const bool boundary = last || h->ops[sched[k + 1].op].kind != h->ops[sched[k].op].kind ||
                                  (h->ops[sched[k].op].kind == OP_CONV && h->ops[sched[k].op].conv == 71 &&
                                   h->ops[sched[k + 1].op].conv != 71);
            if (!h->t_coarse) {
                h->t_slot_op.push_back(sched[k].op);
            } else if (boundary) {
                h->t_slot_op.push_back(seg_first);           // the whole run of same-kind ops is credited to its first op
                if (!last) seg_first = sched[k + 1].op;
            } else {
                h->t_rec[k] = 0;
            }
        }
        h->t_slot_op.push_back((int)h->ops.size());
        h->t_slot_op.push_back((int)h->ops.size() + 1);
    }
    if (ev && n != h->t_n) ev = nullptr;                                   // a session times steps of one batch size
    h->t_recorded_this_call = ev != nullptr;
    int i = 0;
    if (ev) Y4_CHECK_HIP(hipEventRecord(ev[0], s));
    for (size_t k = 0; k < sched.size(); ++k) {
        const Launch& l = sched[k];
        if (int r = run_op(h, l.op, imgs, l.cnt, s, l.img0)) return r;
        if (ev && h->t_rec[k]) Y4_CHECK_HIP(hipEventRecord(ev[++i], s));
    }
    if (int r = detect_tail(h, "y4_predict", nullptr, n, -1.f, -1.f, 0, nullptr, NmsOutputs{boxes, scores, classes, valid, kept_idx}, nullptr, s,
                            ev ? ev[i + 1] : nullptr))
        return r;
    if (ev) Y4_CHECK_HIP(hipEventRecord(ev[i += 2], s));
    return Y4_OK;
}

static int predict_any(y4_handle h, const void* imgs, bool u8, int n, float* boxes, float* scores, float* classes, int32_t* valid,
                       int32_t* kept_idx, void* stream) {
    if (int r = check_handle(h)) return r;
    hipEvent_t* ev = nullptr;
    if (h->t_max_steps > 0 && h->t_steps < h->t_max_steps) ev = h->t_events.data() + (size_t)h->t_steps * h->t_per_step;
    h->img_u8 = u8;
    const int rc = predict_impl(h, imgs, n, boxes, scores, classes, valid, kept_idx, (hipStream_t)stream, ev);
    h->img_u8 = false;
    if (ev && rc == Y4_OK && h->t_recorded_this_call) ++h->t_steps;
    return rc;
}

int y4_predict(y4_handle h, const float* imgs, int n, float* boxes, float* scores, float* classes, int32_t* valid,
               int32_t* kept_idx, void* stream) {
    return predict_any(h, imgs, false, n, boxes, scores, classes, valid, kept_idx, stream);
}
int y4_predict_u8(y4_handle h, const uint8_t* imgs, int n, float* boxes, float* scores, float* classes, int32_t* valid,
                  int32_t* kept_idx, void* stream) {
    return predict_any(h, imgs, true, n, boxes, scores, classes, valid, kept_idx, stream);
}

// Per-layer tile choice by measurement: every tile configuration that fits a conv is timed on the layer's
// real shape (HIP events on `stream`, whatever data is in the workspace) and the fastest is kept.  All tiles
// produce bit-identical results (same K order), so this changes speed only.
// With a second handle `h2` (a sibling: same plan, own workspace; y4_autotune_pair) every timed launch is issued on BOTH
// handles, each on its own stream, and the time until both streams are done is what counts: the objective becomes
// throughput with two batches in flight -- a tile whose last round leaves compute units idle no longer pays for them (the
// other stream fills them), so what wins is the least work, not the shortest solitary launch.  Both handles end up with
// the same choices.
static int autotune_impl(y4_handle h, y4_handle h2, int n, int reps, hipStream_t s, hipStream_t s2, int pair_passes) {
    if (int r = check_ready(h, n)) return r;
    if (h2)
        if (int r = check_ready(h2, n)) return r;
    Y4_REQUIRE(reps >= 1 && reps <= 100, Y4_EINVAL, "y4_autotune: reps %d", reps);
    Y4_REQUIRE(!h2 || (h2 != h && same_plan(h, h2) && s2 != s), Y4_EINVAL,
               "y4_autotune_pair: the second handle must be a sibling of the first (same plan) on another stream");
    hipEvent_t e0, e1, e2;
    Y4_CHECK_HIP(hipEventCreate(&e0));
    Y4_CHECK_HIP(hipEventCreate(&e1));
    Y4_CHECK_HIP(hipEventCreate(&e2));
    int rc = Y4_OK;
    const int ntiles = conv_tile_count();
    // one op on the first handle, and on the second (its own stream) in the passes that use the two-stream objective
    // (pair_passes bit 0: tiles, 1: chains / LDS pairs, 2: stage kernel, 3: residual-block kernels)
    bool two = false;
    auto run_both = [&](int oi, int ne, bool chained) -> int {
        int r = run_op(h, oi, nullptr, ne, s, 0, chained);
        if (r == Y4_OK && two) r = run_op(h2, oi, nullptr, ne, s2, 0, chained);
        return r;
    };
    // the timed region: e0 on s (s2 starts behind it), the launches, then s waits for s2's tail and e1 closes it
    auto t_begin = [&]() -> bool {
        if (hipEventRecord(e0, s) != hipSuccess) return false;
        return !two || hipStreamWaitEvent(s2, e0, 0) == hipSuccess;
    };
    auto t_end = [&](float* ms) -> bool {
        if (two && (hipEventRecord(e2, s2) != hipSuccess || hipStreamWaitEvent(s, e2, 0) != hipSuccess)) return false;
        return hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
               hipEventElapsedTime(ms, e0, e1) == hipSuccess;
    };
    // time `reps` launches of one op; < 0: this tile does not fit, -2: HIP failure
    // Latency schedules (y4_set_splitk) are timed COLD: in a step of one image a layer finds its weights in no L2 (the other 109
    // layers' weights went through since), and the long serial K loop of a few-tile launch is exactly what that hurts -- back to
    // back the same launch runs on warm weights and the unsplit tile looks as good as the split one.  So every timed launch is
    // preceded by a pass of <= 64 MB of the packed weights through the L2s, outside its event pair.
    // (Y4_TUNE_COLD=1: cold timing for throughput schedules too -- an experiment switch, scripts/sched_ab_headline.sh)
    static const bool force_cold = [] { const char* e = getenv("Y4_TUNE_COLD"); return e && e[0] == '1'; }();
    const bool cold = (h->allow_splitk && !h2) || (force_cold && !h2);
    const size_t flush_bytes = h->wts_bytes < ((size_t)64 << 20) ? h->wts_bytes : ((size_t)64 << 20);
    auto time_op = [&](int oi, int ne, bool chained) -> float {
        if (run_both(oi, ne, chained) != Y4_OK) return -1.f;
        if (cold) {
            float total = 0.f;
            for (int i = 0; i < reps; ++i) {
                if (l2_flush_launch(h->wts, flush_bytes, h->act + h->scratch_off, s) != Y4_OK) return -2.f;
                if (hipEventRecord(e0, s) != hipSuccess) return -2.f;
                run_both(oi, ne, chained);
                float ms = 0.f;
                if (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
                    return -2.f;
                total += ms;
            }
            return total;
        }
        if (!t_begin()) return -2.f;
        for (int i = 0; i < reps; ++i) run_both(oi, ne, chained);
        float ms = 0.f;
        return t_end(&ms) ? ms : -2.f;
    };
    // Final decision of passes 2-4, head to head, each variant as the executor would run it: `once(fused)` issues the variant's
    // launches once (the separate kernels in their real order, not the same kernel back to back, which runs warmer than it ever
    // does in a step).  One untimed block of max(reps, 3) of them each way (both start equally warm), then 4 alternating timed
    // blocks.  Comparing a fused probe with the SUM of per-tile minima instead is biased towards "separate" (a minimum of noisy
    // samples is low, and several of them add up) and flipped the 8 % wins of the 76^2 pairs run to run.
    // -> Y4_EHIP (an event failure is not "fused lost"), Y4_EINVAL when the separate kernels themselves fail (their launch's
    // message stays, y4_last_error), else Y4_OK and the verdict; a failing fused launch loses rather than "win" with ~0 ms.
    const int per_block = reps > 3 ? reps : 3;
    auto head_to_head = [&](const auto& once, bool* fused_wins) -> int {
        auto block = [&](bool fused) -> float {            // ms; -2: HIP failure, -1: a launch failed
            if (!t_begin()) return -2.f;
            for (int i = 0; i < per_block; ++i)
                if (once(fused) != Y4_OK) return -1.f;
            float ms = 0.f;
            return t_end(&ms) ? ms : -2.f;
        };
        const float w_f = block(true), w_s = block(false);
        if (w_f == -2.f || w_s == -2.f) return Y4_EHIP;
        bool fused_ok = w_f >= 0.f, sep_ok = w_s >= 0.f;
        float t_fused = 0.f, t_sep = 0.f;
        for (int r = 0; r < 4 && fused_ok && sep_ok; ++r) {
            const float a = block(true), b = block(false);
            if (a == -2.f || b == -2.f) return Y4_EHIP;
            fused_ok = a >= 0.f; sep_ok = b >= 0.f;
            t_fused += a; t_sep += b;
        }
        if (!sep_ok) return Y4_EINVAL;
        *fused_wins = fused_ok && t_fused < t_sep;
        return Y4_OK;
    };
    // every choice is made on both handles: the sibling ends up with the same schedule
    auto choose = [&](const auto& write) {
        write(h->sched);
        if (h2) write(h2->sched);
    };
    auto force_chain = [&](int ci) { h->force_chain = ci; if (h2) h2->force_chain = ci; };
    const Schedule& sc = h->sched;
    auto images_of = [&](int oi) { return (sc.sub_images > 0 && oi <= sc.sub_last_op && n > sc.sub_images) ? sc.sub_images : n; };
    // passes 1 and 2 tune the stage's convs as separate kernels, pass 3 decides; likewise the residual-block kernels: pass 4
    choose([](Schedule& x) { x.stage_enabled = x.res_enabled[0] = x.res_enabled[1] = false; });
    // pass 1: every conv as its own kernel
    two = h2 && (pair_passes & 1);
    for (int oi = 0; oi < (int)h->ops.size() && rc == Y4_OK; ++oi) {
        const Op& op = h->ops[oi];
        if (op.kind != OP_CONV || (sc.fuse_stem && op.conv == 1)) continue;
        float best = 1e30f;
        int best_tile = 0;
        for (int tile = 1; tile <= ntiles; ++tile) {
            // the 32x32x16-MFMA tiles sum in another order than all the others: offering them here would make the outputs
            // depend on the tuner's choice.  They are measured slower anyway (LABNOTES.md section 4.1) and stay explicit-only.
            if (tuner_skips_tile(tile) && !(sc.allow_halo2 && halo2_tile(tile))) continue;
            choose([&](Schedule& x) { x.tile[oi] = tile; });
            const float ms = time_op(oi, images_of(oi), false);
            if (ms == -2.f) { rc = Y4_EHIP; break; }
            if (ms >= 0.f && ms < best) { best = ms; best_tile = tile; }
        }
        // latency schedules (y4_set_splitk): the same tiles with their K loop split 2 / 4 / 8 ways; the launcher refuses the ids
        // that do not fit the layer (too few K-tiles, too many output tiles for the scratch), which reads as "does not fit" here
        if (h->allow_splitk && rc == Y4_OK)
            for (int tile = 1; tile <= ntiles && rc == Y4_OK; ++tile) {
                if (tuner_skips_tile(tile) || !splitk_tile(tile)) continue;
                for (int e = 1; e <= SPLITK_MAX_E; ++e) {
                    choose([&](Schedule& x) { x.tile[oi] = tile + 100 * e; });
                    const float ms = time_op(oi, images_of(oi), false);
                    if (ms == -2.f) { rc = Y4_EHIP; break; }
                    if (ms < 0.f) break;                       // a wider split of this tile will not fit either
                    if (ms < best) { best = ms; best_tile = tile + 100 * e; }
                }
            }
        choose([&](Schedule& x) { x.tile[oi] = best_tile; });
    }
    // pass 2: each chain as one kernel against its separate kernels
    two = h2 && (pair_passes & 2);
    for (int ci = 0; sc.fuse_chains && ci < (int)h->chains.size() && rc == Y4_OK; ++ci) {
        const Chain& ch = h->chains[ci];
        // an alternative run is timed as if its parent's head sat in a residual-block kernel (those are off until pass 4)
        force_chain(ch.alt_of >= 0 ? ci : -1);
        float best = 1e30f;
        int best_tile = 0;
        for (int tile = 1; tile <= ntiles; ++tile) {
            choose([&](Schedule& x) { x.run[ci] = {true, tile}; });
            const float ms = time_op(ch.head, images_of(ch.head), true);
            if (ms == -2.f) { rc = Y4_EHIP; break; }
            if (ms >= 0.f && ms < best) { best = ms; best_tile = tile; }
        }
        choose([&](Schedule& x) { x.run[ci] = {best_tile > 0, best_tile}; });
        if (!sc.run[ci].enabled || rc != Y4_OK) continue;
        bool wins = false;
        rc = head_to_head([&](bool fused) -> int {
            if (fused) return run_both(ch.head, images_of(ch.head), true);
            for (int oi : {ch.head, ch.tail[0], ch.tail[1]})
                if (oi >= 0)
                    if (int r = run_both(oi, images_of(oi), false)) return r;
            return Y4_OK;
        }, &wins);
        if (rc == Y4_OK) choose([&](Schedule& x) { x.run[ci].enabled = wins; });     // (on a failure the run stays as its tile probe left it)
    }
    force_chain(-1);
    // pass 3: the stage kernel (convs 2..7 in one launch) head to head against the same ops as tuned above
    two = h2 && (pair_passes & 4);
    if (rc == Y4_OK && h->stage_first >= 0 && sc.stage_on) {
        const int ne = images_of(h->stage_first);
        bool wins = false;
        rc = head_to_head([&](bool fused) -> int {
            choose([&](Schedule& x) { x.stage_enabled = fused; });
            for (int oi = h->stage_first; oi <= h->stage_last; ++oi)
                if (int r = run_both(oi, ne, true)) return r;
            return Y4_OK;
        }, &wins);
        choose([&](Schedule& x) { x.stage_enabled = rc == Y4_OK && wins; });
    }
    // pass 4: per channel group, the residual blocks as one kernel each against the same op range as tuned above
    two = h2 && (pair_passes & 8);
    for (int grp = 0; grp < 2 && rc == Y4_OK && sc.res_on; ++grp) {
        int lo = -1, hi = -1;
        for (const ResRun& r : h->resruns)
            if ((r.c == 128 ? 0 : 1) == grp) { if (lo < 0) lo = r.head; hi = r.tail; }
        if (lo < 0) continue;
        // include the ops up to the end of the stage's residual chain consumers that existing chains may have fused with it
        for (const Chain& ch : h->chains)
            if (ch.head >= lo && ch.head <= hi) { if (ch.tail[0] > hi) hi = ch.tail[0]; if (ch.tail[1] > hi) hi = ch.tail[1]; }
        const int ne = images_of(lo);
        bool wins = false;
        rc = head_to_head([&](bool fused) -> int {
            choose([&](Schedule& x) { x.res_enabled[grp] = fused; });
            for (int oi = lo; oi <= hi; ++oi)
                if (int r = run_both(oi, ne, true)) return r;
            return Y4_OK;
        }, &wins);
        choose([&](Schedule& x) { x.res_enabled[grp] = rc == Y4_OK && wins; });
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipEventDestroy(e2);
    if (rc == Y4_EHIP) set_error("y4_autotune: HIP event failure");     // (Y4_EINVAL: the failing launch's own message stays)
    return rc;
}

int y4_autotune(y4_handle h, int n, int reps, void* stream) { return autotune_impl(h, nullptr, n, reps, (hipStream_t)stream, nullptr, 0); }

int y4_autotune_pair(y4_handle h, y4_handle h2, int n, int reps, void* stream, void* stream2, int pair_passes) {
    if (int r = check_handle(h2)) return r;
    Y4_REQUIRE(pair_passes >= 0 && pair_passes <= 15, Y4_EINVAL, "y4_autotune_pair: pair_passes %d (bits 0..3)", pair_passes);
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(same_switches(h->sched, h2->sched) && h2->alias_bufs == h->alias_bufs, Y4_ESTATE,
               "y4_autotune_pair: the two handles differ in their fusion switches, sub-batching or workspace aliasing "
               "(y4_copy_schedule(h, h2) makes them equal)");
    return autotune_impl(h, h2, n, reps, (hipStream_t)stream, (hipStream_t)stream2, pair_passes);
}

int y4_set_tiles(y4_handle h, const int32_t* tiles, int count) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(tiles && count == (int)h->layers.size(), Y4_EINVAL, "y4_set_tiles: expected %d entries", (int)h->layers.size());
    Schedule& sc = h->sched;
    for (int oi = 0; oi < (int)h->ops.size(); ++oi) {
        const Op& op = h->ops[oi];
        if (op.kind != OP_CONV) continue;
        const int v = tiles[op.conv];
        int head_of = -1;
        for (int ci = 0; ci < (int)h->chains.size(); ++ci)
            if (h->chains[ci].head == oi) head_of = ci;
        const bool is_head = head_of >= 0 && sc.fuse_chains;
        const TileEntry e = decode_entry(v);
        Y4_REQUIRE(tile_id_ok(e.own) && e.run <= conv_tile_count() && (v >= 0 || is_head), Y4_EINVAL,
                   "y4_set_tiles: tile id %d for conv %d", v, op.conv);
        if (is_head) sc.run[head_of] = {e.chained, e.run};       // (a plain -t leaves the stand-alone tile below as it is)
        if (!is_head || v > 0 || e.own > 0) sc.tile[oi] = e.own;
    }
    return Y4_OK;
}

int y4_set_subbatch(y4_handle h, int images, int last_conv) {
    if (int r = check_settable(h, "y4_set_subbatch")) return r;
    Y4_REQUIRE(images <= 0 || !h->alias_bufs, Y4_ESTATE, "y4_set_subbatch: not together with workspace aliasing (a sub-batch's "
               "early tensors would share memory with another sub-batch's later ones)");
    if (images <= 0) { h->sched.sub_images = 0; h->sched.sub_last_op = -1; return Y4_OK; }
    int last_op = -1;
    for (int i = 0; i < (int)h->ops.size(); ++i)
        if (h->ops[i].kind != OP_SPP && (h->ops[i].conv == last_conv || h->ops[i].conv2 == last_conv)) last_op = i;
    Y4_REQUIRE(last_op >= 0, Y4_EINVAL, "y4_set_subbatch: no conv %d", last_conv);
    h->sched.sub_images = images; h->sched.sub_last_op = last_op;
    return Y4_OK;
}

int y4_set_stem_fusion(y4_handle h, int on) {
    if (int r = check_settable(h, "y4_set_stem_fusion")) return r;
    if (on) {
        const bool shape_ok = h->ops.size() > 1 && h->ops[0].kind == OP_STEM && h->ops[1].kind == OP_CONV &&
                              h->ops[1].conv == 1 && h->ops[1].conv2 < 0 && !h->ops[1].has_res &&
                              h->layers[0].d.cout == 32 && h->layers[1].d.cout == 64 && h->layers[1].d.ksize == 3 &&
                              h->layers[1].d.stride == 2;
        // stem_down.hip walks a square image (one side S for rows and columns): a rectangular handle runs convs 0 and 1 apart
        Y4_REQUIRE(h->H == h->W, Y4_EINVAL, "y4_set_stem_fusion: square inputs only (this handle is %d x %d); convs 0 and 1 run as "
                   "separate kernels", h->H, h->W);
        Y4_REQUIRE(shape_ok && stem_down_supported(h->cfg.dtype, h->H), Y4_EINVAL,
                   "y4_set_stem_fusion: needs a 16-bit dtype and img_size <= 640 (dtype %d, img_size %d)", h->cfg.dtype, h->H);
    }
    h->sched.fuse_stem = on != 0;
    return Y4_OK;
}

int y4_set_chain_fusion(y4_handle h, int on) {
    if (int r = check_settable(h, "y4_set_chain_fusion")) return r;
    Y4_REQUIRE(!on || h->cfg.dtype != Y4_F32, Y4_EINVAL, "y4_set_chain_fusion: 16-bit dtypes only");
    h->sched.fuse_chains = on != 0;
    h->sched.run.assign(h->chains.size(), Schedule::Run{});
    return on ? (int)h->chains.size() : Y4_OK;
}

int y4_set_stage_fusion(y4_handle h, int on) {
    if (int r = check_settable(h, "y4_set_stage_fusion")) return r;
    Y4_REQUIRE(!on || h->stage_first >= 0, Y4_EINVAL, "y4_set_stage_fusion: needs a 16-bit dtype (dtype %d)", h->cfg.dtype);
    h->sched.stage_on = on != 0;
    h->sched.stage_enabled = true;
    return h->stage_active() ? 1 : 0;
}

int y4_set_res_fusion(y4_handle h, int on) {
    if (int r = check_settable(h, "y4_set_res_fusion")) return r;
    Y4_REQUIRE(!on || h->cfg.dtype != Y4_F32, Y4_EINVAL, "y4_set_res_fusion: 16-bit dtypes only");
    h->sched.res_on = on != 0;
    h->sched.res_enabled[0] = h->sched.res_enabled[1] = true;
    return on ? (int)h->resruns.size() : Y4_OK;
}

int y4_get_res_fusion(y4_handle h) {
    if (int r = check_handle(h)) return r;
    if (!h->sched.res_on) return 0;
    int mask = 0;
    for (const ResRun& r : h->resruns) mask |= h->sched.res_enabled[r.c == 128 ? 0 : 1] ? (r.c == 128 ? 1 : 2) : 0;
    return mask;
}

int y4_set_res_fusion_mask(y4_handle h, int mask) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(h->cfg.dtype != Y4_F32 || mask == 0, Y4_EINVAL, "y4_set_res_fusion_mask: 16-bit dtypes only");
    Y4_REQUIRE(mask >= 0 && mask <= 3, Y4_EINVAL, "y4_set_res_fusion_mask: mask %d (bit 0: 128-channel blocks, bit 1: 64-channel blocks)", mask);
    if (int r = check_settable(h, "y4_set_res_fusion_mask")) return r;
    h->sched.res_on = mask != 0;
    h->sched.res_enabled[0] = (mask & 1) != 0;
    h->sched.res_enabled[1] = (mask & 2) != 0;
    return Y4_OK;
}

int y4_rb_tile_table(int32_t n, int32_t h, int32_t w, int32_t c, int32_t slots, int32_t* out, int32_t cap) {
    return rb_tile_table(n, h, w, c, slots, out, cap);
}

int y4_set_splitk(y4_handle h, int on) {
    if (int r = check_handle(h)) return r;
    h->allow_splitk = on != 0;
    return Y4_OK;
}

int y4_set_halo2(y4_handle h, int on) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(!on || h->cfg.dtype != Y4_F32, Y4_EINVAL, "y4_set_halo2: 16-bit dtypes only");
    h->sched.allow_halo2 = on != 0;
    return Y4_OK;
}

int y4_get_stage_fusion(y4_handle h) {
    if (int r = check_handle(h)) return r;
    return h->stage_active() ? 1 : 0;
}

int y4_get_tiles(y4_handle h, int32_t* tiles, int cap) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(tiles && cap >= (int)h->layers.size(), Y4_EINVAL, "y4_get_tiles: need room for %d layers", (int)h->layers.size());
    for (int i = 0; i < (int)h->layers.size(); ++i) tiles[i] = 0;
    const Schedule& sc = h->sched;
    for (int oi = 0; oi < (int)h->ops.size(); ++oi) {
        const Op& op = h->ops[oi];
        if (op.kind != OP_CONV) continue;
        tiles[op.conv] = sc.tile[oi];
        if (op.conv2 >= 0) tiles[op.conv2] = sc.tile[oi];
    }
    for (int ci = 0; sc.fuse_chains && ci < (int)h->chains.size(); ++ci) {      // a chained run's head: both tiles (TileEntry)
        const int head = h->chains[ci].head;
        if (sc.run[ci].enabled) tiles[h->ops[head].conv] = encode_entry(sc.run[ci].tile, sc.tile[head]);
    }
    return Y4_OK;
}

// Every scheduling choice of `src` -> `dst` (a sibling built from the same configuration): the whole Schedule.
int y4_copy_schedule(y4_handle src, y4_handle dst) {
    if (int r = check_handle(src)) return r;
    if (int r = check_handle(dst)) return r;
    Y4_REQUIRE(src != dst, Y4_EINVAL, "y4_copy_schedule: source and destination are the same handle");
    Y4_REQUIRE(dst->t_max_steps == 0, Y4_ESTATE, "y4_copy_schedule: a timing session is open on the destination");
    Y4_REQUIRE(same_plan(src, dst), Y4_EINVAL, "y4_copy_schedule: the handles were not created from the same configuration");
    Y4_REQUIRE(src->sched.sub_images <= 0 || !dst->alias_bufs, Y4_ESTATE,
               "y4_copy_schedule: the source runs sub-batches, the destination's workspace is aliased");
    dst->sched = src->sched;
    return Y4_OK;
}

int y4_launch_counts(y4_handle h, int32_t* conv_family, int32_t* total) {
    if (int r = check_handle(h)) return r;
    int convs = 0, all = 2;                                  // decode + nms
    for (int oi = 0; oi < (int)h->ops.size(); ++oi) {
        if (resolve_op(h, oi, true).kind == EX_SKIP) continue;
        ++all;
        if (h->ops[oi].kind == OP_CONV) ++convs;
    }
    if (conv_family) *conv_family = convs;
    if (total) *total = all;
    return Y4_OK;
}

int y4_timing_begin(y4_handle h, int max_steps, int coarse) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(max_steps >= 1 && max_steps <= 4096, Y4_EINVAL, "y4_timing_begin: max_steps %d", max_steps);
    Y4_REQUIRE(h->t_max_steps == 0, Y4_ESTATE, "a timing session is already open");
    h->t_coarse = coarse != 0;
    {
        std::vector<Launch> sched;
        build_schedule(h, h->cfg.max_batch, sched);
        h->t_per_step = (int)sched.size() + 3;
    }
    h->t_events.resize((size_t)max_steps * h->t_per_step);
    for (auto& e : h->t_events) Y4_CHECK_HIP(hipEventCreate(&e));
    h->t_max_steps = max_steps;
    h->t_steps = 0;
    return Y4_OK;
}

int y4_timing_end(y4_handle h, float* op_ms_mean, char* names, int cap, int* n_ops, int* steps, void* stream) {
    if (int r = check_handle(h)) return r;
    Y4_REQUIRE(h->t_max_steps > 0, Y4_ESTATE, "no timing session is open");
    const int nops = (int)h->ops.size() + 2;
    int rc = Y4_OK;
    if (!op_ms_mean || !n_ops || cap < nops) {
        set_error("y4_timing_end: need room for %d ops", nops);
        rc = Y4_EINVAL;
    }
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == Y4_OK) {
        set_error("y4_timing_end: stream synchronize failed");
        rc = Y4_EHIP;
    }
    if (rc == Y4_OK) {
        std::vector<double> acc(nops, 0.0);
        for (int st = 0; st < h->t_steps; ++st) {
            hipEvent_t* ev = h->t_events.data() + (size_t)st * h->t_per_step;
            for (int k = 0; k < (int)h->t_slot_op.size(); ++k) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) != hipSuccess) { rc = Y4_EHIP; set_error("hipEventElapsedTime failed"); }
                acc[h->t_slot_op[k]] += ms;          // a sub-batched op has several slots per step
            }
        }
        for (int j = 0; j < nops; ++j) {
            op_ms_mean[j] = h->t_steps ? (float)(acc[j] / h->t_steps) : 0.f;
            if (names) {
                memset(names + 16 * j, 0, 16);
                const char* nm = j < (int)h->ops.size() ? h->ops[j].name : (j == (int)h->ops.size() ? "decode" : "nms");
                strncpy(names + 16 * j, nm, 15);
            }
        }
        *n_ops = nops;
        if (steps) *steps = h->t_steps;
    }
    for (auto& e : h->t_events) (void)hipEventDestroy(e);
    h->t_events.clear();
    h->t_max_steps = 0;
    h->t_steps = 0;
    return rc;
}

// One forward + decode + NMS with per-op HIP-event timing (synchronises): a one-step timing session.
int y4_profile(y4_handle h, const float* imgs, int n, float* op_ms, char* names, int cap, int* n_ops, void* stream) {
    if (int r = check_ready(h, n)) return r;
    Y4_REQUIRE(imgs && op_ms && n_ops, Y4_EINVAL, "y4_profile: null argument");
    if (int r = y4_timing_begin(h, 1, 0)) return r;
    float* boxes = (float*)(h->act + h->scratch_off);
    float* scores = boxes + (size_t)n * h->cfg.max_total * 4;
    float* classes = scores + (size_t)n * h->cfg.max_total;
    int32_t* kept = (int32_t*)(classes + (size_t)n * h->cfg.max_total);
    int32_t* valid = kept + (size_t)n * h->cfg.max_total;
    const int rc = y4_predict(h, imgs, n, boxes, scores, classes, valid, kept, stream);
    const int rc2 = y4_timing_end(h, op_ms, names, cap, n_ops, nullptr, stream);
    return rc ? rc : rc2;
}

// ---------------------------------------------------------------- standalone operators
int y4_packed_conv_bytes(int dtype, int cout, int cin, int ksize, int32_t* cout_pad, size_t* bytes) {
    Y4_REQUIRE(dtype >= Y4_F32 && dtype <= Y4_F16 && cout > 0 && cin > 0 && (ksize == 1 || ksize == 3), Y4_EINVAL,
               "y4_packed_conv_bytes: bad argument");
    const int cp = (int)round_up(cout, COUT_PAD);
    if (cout_pad) *cout_pad = cp;
    if (bytes) *bytes = (size_t)cp * ksize * ksize * cin * elem_size(dtype);
    return Y4_OK;
}

int y4_pack_conv_weights(int dtype, int cout, int cin, int ksize, const float* oihw_dev, void* packed_dev, void* stream) {
    Y4_REQUIRE(oihw_dev && packed_dev, Y4_EINVAL, "y4_pack_conv_weights: null pointer");
    return pack_conv_weights(dtype, cout, cin, ksize, oihw_dev, packed_dev, (hipStream_t)stream);
}

int y4_pack_conv_frag32(int dtype, int cout, int cin, const void* packed_dev, void* frag_dev, void* stream) {
    Y4_REQUIRE(packed_dev && frag_dev, Y4_EINVAL, "y4_pack_conv_frag32: null pointer");
    return pack_conv_frag32(dtype, cout, cin, packed_dev, frag_dev, (hipStream_t)stream);
}

static char* g_zero_page = nullptr;
int y4_conv2d(const y4_conv_desc* d, void* stream) {
    if (!g_zero_page) {
        Y4_CHECK_HIP(hipMalloc((void**)&g_zero_page, ZERO_PAGE_BYTES));
        Y4_CHECK_HIP(hipMemset(g_zero_page, 0, ZERO_PAGE_BYTES));
    }
    return conv2d_launch(d, g_zero_page, (hipStream_t)stream);
}
int y4_conv_tile_count(void) { return conv_tile_count(); }

int y4_conv_tile_desc(int tile, int32_t cfg[6]) {
    Y4_REQUIRE(cfg && tile >= 1 && tile <= conv_tile_count(), Y4_EINVAL, "y4_conv_tile_desc: tile %d", tile);
    const TileCfg& t = kTiles[tile - 1];
    cfg[0] = t.bm; cfg[1] = t.bn; cfg[2] = t.wm; cfg[3] = t.wn; cfg[4] = t.bkb; cfg[5] = t.nst;
    return Y4_OK;
}

int y4_pack_stem_weights(const float* w_oihw_dev, float* wk_dev, int cout, void* stream) {
    return pack_stem_weights(w_oihw_dev, wk_dev, cout, (hipStream_t)stream);
}

int y4_stem_conv(int dtype, const float* imgs_dev, int n, int h, int w, const float* wk_dev, const float* scale,
                 const float* shift, int cout, int act, void* out_dev, int out_cstride, int out_coff, void* stream) {
    return stem_conv_launch(dtype, imgs_dev, 0, n, h, w, wk_dev, scale, shift, cout, act, out_dev, out_cstride,
                            out_coff, (hipStream_t)stream);
}

int y4_resize_u8(const uint8_t* imgs_dev, int n, int h, int w, uint8_t* out_dev, int out_h, int out_w, void* stream) {
    return resize_u8_launch(imgs_dev, n, h, w, out_dev, out_h, out_w, (hipStream_t)stream);
}

int y4_resize_u8_ragged(const uint8_t* src_dev, const y4_image_desc* desc_dev, int n, uint8_t* out_dev, int H, int W,
                        int pad_value, void* stream) {
    return resize_u8_ragged_launch(src_dev, desc_dev, n, out_dev, H, W, pad_value, (hipStream_t)stream);
}

int y4_window_u8_ragged(const uint8_t* src_dev, const y4_window_desc* desc_dev, int n, uint8_t* out_dev, int H, int W,
                        int pad_value, void* stream) {
    return window_u8_ragged_launch(src_dev, desc_dev, n, out_dev, H, W, pad_value, (hipStream_t)stream);
}

int y4_view_u8_ragged(const uint8_t* src_dev, const y4_view_desc* desc_dev, int n, uint8_t* out_dev, int H, int W, int pad_value,
                      void* stream) {
    return view_u8_ragged_launch(src_dev, desc_dev, n, out_dev, H, W, pad_value, (hipStream_t)stream);
}

int y4_augment_u8_ragged(const uint8_t* src_dev, const y4_augment_desc* desc_dev, int n, uint8_t* out_dev, int H, int W,
                         int pad_value, void* stream) {
    return augment_u8_ragged_launch(src_dev, desc_dev, n, out_dev, H, W, pad_value, (hipStream_t)stream);
}

int y4_mosaic_u8_ragged(const uint8_t* src_dev, const y4_augment_desc* tiles_dev, const y4_mosaic_cut* cuts_dev, int n,
                        uint8_t* out_dev, int H, int W, int pad_value, void* stream) {
    return mosaic_u8_ragged_launch(src_dev, tiles_dev, cuts_dev, n, out_dev, H, W, pad_value, (hipStream_t)stream);
}

int y4_yuv_u8_ragged(const uint8_t* src_dev, const y4_yuv_desc* desc_dev, int n, uint8_t* out_dev, int H, int W, int pad_value,
                     void* stream) {
    return yuv_u8_ragged_launch(src_dev, desc_dev, n, out_dev, H, W, pad_value, (hipStream_t)stream);
}

int y4_map_match(const float* boxes_dev, const float* scores_dev, const float* classes_dev, const int32_t* valid_dev, int n,
                 int max_total, const float* scale_dev, const float* gt_dev, const int32_t* gt_count_dev, int max_gt,
                 const double* iou_thresholds, int n_thresholds, uint32_t* tp_mask_dev, double* best_iou_dev, int32_t* match_dev,
                 uint32_t* gt_used_dev, void* stream) {
    return map_match_launch(boxes_dev, scores_dev, classes_dev, valid_dev, n, max_total, scale_dev, gt_dev, gt_count_dev, max_gt,
                            iou_thresholds, n_thresholds, tp_mask_dev, best_iou_dev, match_dev, gt_used_dev, (hipStream_t)stream);
}

int y4_coco_match(const float* boxes_dev, const float* scores_dev, const float* classes_dev, const int32_t* valid_dev, int n,
                  int max_total, const float* scale_dev, const float* gt_dev, const int32_t* gt_count_dev, int max_gt,
                  const double* area_ranges, int n_areas, const double* iou_thresholds, int n_thresholds, uint32_t* dt_match_dev,
                  uint32_t* dt_ignore_dev, int32_t* cls_rank_dev, uint32_t* gt_ignore_dev, int32_t* match_row_dev, void* stream) {
    return coco_match_launch(boxes_dev, scores_dev, classes_dev, valid_dev, n, max_total, scale_dev, gt_dev, gt_count_dev, max_gt,
                             area_ranges, n_areas, iou_thresholds, n_thresholds, dt_match_dev, dt_ignore_dev, cls_rank_dev,
                             gt_ignore_dev, match_row_dev, (hipStream_t)stream);
}

int y4_anchor_step(const float* wh_dev, int n, const float* anchors_dev, int k, float* next_dev, int64_t* stats_dev,
                   uint8_t* assign_dev, void* stream) {
    return anchor_step_launch(wh_dev, n, anchors_dev, k, next_dev, stats_dev, assign_dev, (hipStream_t)stream);
}

int y4_anchor_fitness(const float* wh_dev, int n, const float* sets_dev, int P, int k, int64_t* f_dev, void* stream) {
    return anchor_fitness_launch(wh_dev, n, sets_dev, P, k, f_dev, (hipStream_t)stream);
}

int y4_anchor_evolve(const float* wh_dev, int n, float* best_dev, int64_t* fbest_dev, const float* mult_dev, int G, int P, int k,
                     int64_t* fhist_dev, int32_t* accepted_dev, void* stream) {
    return anchor_evolve_launch(wh_dev, n, best_dev, fbest_dev, mult_dev, G, P, k, fhist_dev, accepted_dev, (hipStream_t)stream);
}

int y4_preprocess_u8(const uint8_t* img_dev, int h, int w, float* out_dev, int out_h, int out_w, void* stream) {
    return preprocess_u8_launch(img_dev, h, w, out_dev, out_h, out_w, (hipStream_t)stream);
}

int y4_spp(int dtype, void* buf_dev, int n, int side, int c, void* stream) {
    return spp_launch(dtype, buf_dev, n, side, side, c, (hipStream_t)stream);
}

int y4_spp_hw(int dtype, void* buf_dev, int n, int h, int w, int c, void* stream) {
    return spp_launch(dtype, buf_dev, n, h, w, c, (hipStream_t)stream);
}

}  // extern "C"
