// Layer programs (pp_net_*): a pp_op list over NHWC buffers, checked and planned once at creation, then launched op by op.
// What an op type IS on this side stands in one place: its row of kOpKinds and the check / launch pair the row points at.
#include <algorithm>
#include <memory>

#include "pp_internal.h"
#include "pp_amax.h"

struct pp_net {
    pp_ctx* ctx = nullptr;
    std::vector<pp_op> ops;
    std::vector<pp_buf> bufs;
    std::vector<size_t> buf_off;    // float offset of buffer b (sized for max_batch)
    std::vector<size_t> buf_elems;  // per-sample floats
    float* weights = nullptr;
    size_t n_weights = 0;
    // conv_split_weights.hip: the eligible convs' weights as bf16 planes in fragment order (built on the device at creation)
    unsigned char* wsplit = nullptr;
    std::vector<SplitPlan> split_plan;   // per op, split nets: how the op runs on the split kernels (SPLIT_NONE: the fp32-MFMA kernels)
    int numerics = PP_NET_NUMERICS_EXACT;   // fixed at creation (ABI 7)
    int split_f16 = 0;                      // split nets: the fp16 form (ABI 9), fixed at creation as well
    // fp16 form (pp_amax.h): per-sample running maxima of the tensors its convolutions read, [slot][max_batch] bit patterns.  A slot
    // belongs to ONE tensor of the program (a buffer between two overwrites); it is raised by the fused epilogues of the tensor's
    // producers (op_y_slot) or, where a producer has none, by a stand-alone pass after the last of them (op_post_slot); tensors that
    // come from outside the program (`ext`) get one pass at the start of the run, unless their producer supplies the maxima itself
    // (pp_net_input_amax).  Tensor slots are numbered in op order, so the slots a run of ops [first, last) has to zero are one
    // contiguous range (slot_owner = the first op that raises the slot).
    unsigned* amax = nullptr;
    std::vector<int> op_x_slot, op_y_slot, op_post_slot, slot_owner;
    std::vector<int> op_x2_slot;                 // ... of the second input of an op that carries a folded shortcut (fold_src)
    // projection shortcuts folded into the product they were added to (net_fold_shortcuts; fp16-form nets only).  The op list keeps the
    // caller's numbering: the shortcut op stays in it and is never launched (fold_into[i] = the op that carries it), and the carrying
    // op reads the shortcut's INPUT as a second K segment instead of the shortcut's output as res1 (fold_src[i] = the shortcut op)
    std::vector<int> fold_into, fold_src;
    bool folded(int i) const { return !fold_into.empty() && fold_into[i] >= 0; }
    int carries(int i) const { return fold_src.empty() ? -1 : fold_src[i]; }
    // the buffers op i reads, as executed: {in, res1, res2, in2, in3}
    void reads(int i, int (&r)[5]) const {
        const pp_op& op = ops[i];
        r[0] = op.in; r[1] = op.res1; r[2] = op.res2; r[3] = op.in2; r[4] = op.in3;
        if (folded(i)) r[0] = r[1] = r[2] = r[3] = r[4] = -1;
        else if (carries(i) >= 0) r[1] = ops[carries(i)].in;
    }
    std::vector<int> slot_first, slot_last;      // tracked slots: first / last op that raises them (-1: nobody reads the maxima)
    struct ExtAmax { int buf, slot, first_reader, last_reader; bool provided; };
    std::vector<ExtAmax> ext;      // tensors from outside the program that fp16-form convolutions read
    float* arena = nullptr;
    size_t arena_floats = 0;
    int max_batch = 0;
    hipGraphExec_t graph_exec = nullptr;
    int graph_batch = 0;
    bool use_lanes = true;
    // multi-lane execution: independent ops (HRNet branches, FPN / RPN levels) run on separate HIP streams so
    // that the tail of one launch overlaps the head of another; dependencies (RAW on inputs / residuals, WAR
    // and WAW on recycled buffers) become event waits.
    std::vector<hipStream_t> lanes;
    std::vector<int> op_lane;
    std::vector<std::vector<int>> op_waits;   // ops on OTHER lanes this op must wait for
    std::vector<char> op_needs_event;
    std::vector<hipEvent_t> op_done;
    hipEvent_t fork_ev = nullptr;
    std::vector<hipEvent_t> join_ev;
    std::vector<pp_vit_encoder*> vits;   // per op: the encoder of a PP_OP_VIT_ENCODER, else null
    std::vector<pp_deconv_bf16*> deconvs; // per op: the object of a PP_OP_DECONV_BF16, else null

    pp_net() = default;
    pp_net(const pp_net&) = delete;      // (owns device memory, streams and events)
    ~pp_net();
    void drop_lanes();
    float* buf_ptr(int b) const { return b >= 0 ? arena + buf_off[b] : nullptr; }      // null for "no such operand" (-1)
    unsigned* amax_slot(int slot) const { return slot >= 0 ? amax + (size_t)slot * max_batch : nullptr; }
    // where op i's launch folds the per-sample maximum of what it stores (null: nowhere)
    unsigned* y_amax(int i) const { return amax ? amax_slot(op_y_slot[i]) : nullptr; }
};

// the lane streams and every event of the lane plan (the caller has synchronised them)
void pp_net::drop_lanes() {
    for (auto l : lanes)
        if (l) (void)hipStreamDestroy(l);
    lanes.clear();
    for (auto e : op_done)
        if (e) (void)hipEventDestroy(e);
    op_done.clear();
    for (auto e : join_ev)
        if (e) (void)hipEventDestroy(e);
    join_ev.clear();
    if (fork_ev) (void)hipEventDestroy(fork_ev);
    fork_ev = nullptr;
}

// Everything the net holds, in this order: the streams run dry first, then lanes and events, the graph, the per-op objects, and the
// memory last.  Also the way out of every failed pp_net_create_ex, whose net lives in a unique_ptr: a half-built net has nulls
// (or empty vectors) where it did not get to.
pp_net::~pp_net() {
    if (ctx && ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto l : lanes)
        if (l) (void)hipStreamSynchronize(l);
    drop_lanes();
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    for (auto* v : vits) pp_vit_encoder_destroy(v);
    for (auto* d : deconvs) pp_deconv_bf16_destroy(d);
    if (weights) (void)hipFree(weights);
    if (wsplit) (void)hipFree(wsplit);
    if (amax) (void)hipFree(amax);
    if (arena) (void)hipFree(arena);
}

// ---- op types ------------------------------------------------------------------------------------------------------------------
// One row per pp_op.type.  To add an op type: the constant in posepipe_hip.h (and _lib.py), a ProgramBuilder method that calls
// _emit, and here a row with its check and its launch, written next to each other below.
// fields of pp_op that an op type may not have (they then hold their neutral value) or must have
enum : unsigned { RES1 = 1, RES2 = 2, NCHW = 4, OUT_SLICE = 8, IN_SLICE = 16, UPSAMPLING = 32, IN2 = 64, IN3 = 128, IN23 = IN2 | IN3,
                  ACTIVATION = 256, ACT_BUT_RELU_LAST = 512 };     // (no activation at all; none but PP_RELU_LAST)
struct OpKind {
    const char* name;        // as the messages call it; null: no such op type
    // bi / bo: the op's in and out buffers.  check runs after the shared front of net_check_op
    int (*check)(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo);
    int (*launch)(pp_net* net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s);
    unsigned has_no, needs;  // masks of the fields above (IN2 / IN3 in neither: optional)
    bool halo;               // may touch a buffer with a zero halo (pp_buf.pad): its kernels know the layout
    // (net_plan_amax) the launch folds the per-sample maximum of what it stores into pp_net::y_amax(idx); null: never
    bool (*fused_amax)(pp_net* net, int idx);
    // (net_plan_amax) counts as the writer of a channel slice (op.cout channels) when the fused maxima of a tensor's producers are
    // added up; the others count as writers of the whole buffer.  Other ops CAN write slices; where they do, this decides only
    // whether the tensor's maxima come fused or from a stand-alone pass
    bool slice_writer;
};
static const OpKind& op_kind(int type);

static ConvArgs net_conv_args(pp_net* net, int idx, int batch);
static int net_make_lanes(pp_net* net, int n_lanes);
static void net_fold_shortcuts(pp_net* net);

// which tensors the fp16-form convolutions read, who produces them and who therefore tracks their maxima (see pp_net::amax)
static void net_plan_amax(pp_net* net) {
    const int n = (int)net->ops.size(), nb = (int)net->bufs.size();
    net->op_x_slot.assign(n, -1);
    net->op_y_slot.assign(n, -1);
    net->op_post_slot.assign(n, -1);
    net->op_x2_slot.assign(n, -1);
    net->slot_owner.clear();
    net->ext.clear();
    if (net->numerics != PP_NET_NUMERICS_SPLIT || !net->split_f16) return;
    auto is_h = [&](int i) { return !net->folded(i) && net->ops[i].type == PP_OP_CONV && net->split_plan[i].kernel != SPLIT_NONE; };
    // the k-th tensor op i reads in the fp16 form: its input, and the input of the shortcut folded into it (-1: none)
    auto h_in = [&](int i, int k) { return k == 0 ? net->ops[i].in : net->carries(i) >= 0 ? net->ops[net->carries(i)].in : -1; };
    // producers with a fused maximum: OpKind::fused_amax
    auto tracks = [&](int i) {
        const OpKind& k = op_kind(net->ops[i].type);
        return k.fused_amax && k.fused_amax(net, i);
    };
    // pass 1: buffers a fp16-form convolution reads BEFORE any op of the program has written them = tensors from outside (the
    // program's inputs).  One slot per buffer, numbered first; filled by one stand-alone pass at the start of a run that
    // contains a reader -- or by the caller's own producer (pp_net_input_amax: the detector's RoIAlign)
    {
        std::vector<char> written(nb, 0);
        for (int i = 0; i < n; ++i) {
            const pp_op& op = net->ops[i];
            if (net->folded(i)) continue;             // (never launched: writes nothing)
            for (int k = 0; k < 2; ++k) {
                const int b = h_in(i, k);
                if (!is_h(i) || b < 0 || written[b]) continue;
                pp_net::ExtAmax* e = nullptr;
                for (auto& x : net->ext)
                    if (x.buf == b) e = &x;
                if (!e) {
                    net->ext.push_back({b, (int)net->slot_owner.size(), i, i, false});
                    net->slot_owner.push_back(-1);    // (never part of the zeroed range: handled per run, below)
                    e = &net->ext.back();
                }
                e->last_reader = i;
                (k ? net->op_x2_slot : net->op_x_slot)[i] = e->slot;
            }
            written[op.out] = 1;
        }
    }
    struct Tensor { int slot; std::vector<int> producers; bool wanted; };
    std::vector<Tensor> tensors;
    std::vector<int> cur(nb, -1);                 // tensor currently held by buffer b (-1: written outside the program)
    std::vector<char> read_since(nb, 1);
    struct Reader { int op, tensor, k; };
    std::vector<Reader> readers;                  // (H conv, tensor, which of its inputs)
    for (int i = 0; i < n; ++i) {
        const pp_op& op = net->ops[i];
        if (net->folded(i)) continue;
        for (int k = 0; k < 2; ++k) {
            const int b = h_in(i, k);
            if (!is_h(i) || b < 0 || cur[b] < 0) continue;
            tensors[cur[b]].wanted = true;
            readers.push_back({i, cur[b], k});
        }
        int rd[5];
        net->reads(i, rd);
        for (int b : rd)
            if (b >= 0) read_since[b] = 1;
        // a write after a read (or the first write) starts a new tensor; writes without a read in between fill the same one (the
        // channel slices of a concatenation)
        if (cur[op.out] < 0 || read_since[op.out]) {
            cur[op.out] = (int)tensors.size();
            tensors.push_back({(int)net->slot_owner.size(), {}, false});
            net->slot_owner.push_back(i);         // (a slot per tensor, wanted or not: the numbering must follow the op order)
        }
        tensors[cur[op.out]].producers.push_back(i);
        read_since[op.out] = 0;
    }
    net->slot_first.assign(net->slot_owner.size(), -1);
    net->slot_last.assign(net->slot_owner.size(), -1);
    for (const Tensor& t : tensors) {
        if (!t.wanted) continue;
        net->slot_first[t.slot] = t.producers.front();
        net->slot_last[t.slot] = t.producers.back();
        bool fused = true;
        for (int p : t.producers) fused = fused && tracks(p);
        // the fused maxima cover what the producers WRITE: when their channel slices do not add up to the whole buffer, part of
        // what the readers see is older content (a dense-connection pattern, a buffer partly filled from outside) that only the
        // stand-alone pass over the whole buffer accounts for
        {
            int covered = 0;
            const int out_b = net->ops[t.producers.front()].out;
            for (int p : t.producers)      // the two slice writers: convolutions and PP_OP_BILINEAR_ADD (HRNetv2's resize + concatenate)
                covered += op_kind(net->ops[p].type).slice_writer ? net->ops[p].cout : net->bufs[out_b].c;
            if (covered < net->bufs[out_b].c) fused = false;
        }
        if (fused)
            for (int p : t.producers) net->op_y_slot[p] = t.slot;
        else
            net->op_post_slot[t.producers.back()] = t.slot;
    }
    for (const auto& r : readers) (r.k ? net->op_x2_slot : net->op_x_slot)[r.op] = tensors[r.tensor].slot;
}

// ahead of ops [first, last) on `s`: zero the maxima they raise, and take the maxima of the outside tensors they read
static int net_reset_amax(pp_net* net, int first, int last, int batch, hipStream_t s) {
    if (!net->amax) return PP_OK;
    int s0 = -1, s1 = -1;
    // a range that starts (or ends) between the producers of a tracked tensor would keep (or lose) part of its maxima: the scale
    // would then depend on earlier runs, which the fp16 form promises it never does
    for (int k = 0; k < (int)net->slot_first.size(); ++k) {
        const int a = net->slot_first[k], b = net->slot_last[k];
        if (a < 0 || b < first || a >= last) continue;
        PP_REQUIRE(a >= first && b < last, "pp_net_run: op range [%d, %d) splits the producers (ops %d .. %d) of a tensor whose per-sample maxima are tracked",
                   first, last, a, b);
    }
    for (int k = 0; k < (int)net->slot_owner.size(); ++k)
        if (net->slot_owner[k] >= first && net->slot_owner[k] < last) {
            if (s0 < 0) s0 = k;
            s1 = k + 1;
        }
    if (s0 >= 0) PP_HIP_CHECK(hipMemsetAsync(net->amax_slot(s0), 0, (size_t)(s1 - s0) * net->max_batch * sizeof(unsigned), s));
    for (auto& e : net->ext) {
        if (e.last_reader < first || e.first_reader >= last) continue;
        if (e.provided) {        // the caller's producer filled the slot for THIS run (pp_net_input_amax): a one-shot promise
            e.provided = false;
            continue;
        }
        PP_HIP_CHECK(hipMemsetAsync(net->amax_slot(e.slot), 0, (size_t)batch * sizeof(unsigned), s));
        int rc = pp_launch_amax(net->buf_ptr(e.buf), batch, net->buf_elems[e.buf], net->amax_slot(e.slot), s);
        if (rc != PP_OK) return rc;
    }
    return PP_OK;
}

static void net_plan_lanes(pp_net* net, int n_lanes) {
    const int n = (int)net->ops.size(), nb = (int)net->bufs.size();
    net->op_lane.assign(n, 0);
    net->op_waits.assign(n, {});
    net->op_needs_event.assign(n, 0);
    std::vector<int> last_writer(nb, -1);
    std::vector<std::vector<int>> readers(nb);
    std::vector<int> lane_tail(n_lanes, -1);
    for (int i = 0; i < n; ++i) {
        const pp_op& op = net->ops[i];
        if (net->folded(i)) continue;                   // never launched: no lane, no dependencies, no event
        int rd[5];
        net->reads(i, rd);
        std::vector<int> deps;
        auto add = [&](int d) {
            if (d >= 0 && std::find(deps.begin(), deps.end(), d) == deps.end()) deps.push_back(d);
        };
        for (int b : rd)
            if (b >= 0) add(last_writer[b]);
        add(last_writer[op.out]);                       // WAW
        for (int r : readers[op.out]) add(r);           // WAR
        // lane: continue the lane whose tail is one of the dependencies (largest index), else the stalest lane
        int lane = -1, best = -1;
        for (int l = 0; l < n_lanes; ++l)
            if (lane_tail[l] >= 0 && lane_tail[l] > best && std::find(deps.begin(), deps.end(), lane_tail[l]) != deps.end()) {
                best = lane_tail[l];
                lane = l;
            }
        if (lane < 0) {
            lane = 0;
            for (int l = 1; l < n_lanes; ++l)
                if (lane_tail[l] < lane_tail[lane]) lane = l;
        }
        net->op_lane[i] = lane;
        for (int d : deps)
            if (net->op_lane[d] != lane) {
                net->op_waits[i].push_back(d);
                net->op_needs_event[d] = 1;
            }
        lane_tail[lane] = i;
        for (int b : rd)
            if (b >= 0 && b != op.out) readers[b].push_back(i);
        last_writer[op.out] = i;
        readers[op.out].clear();
    }
}

// ---- conditions that several op types share; each words its message once, with the op's name, and only when it fails -------------
// a parameter block of `floats` floats at float offset `off`: inside the blob and 16-byte aligned
static bool blob_holds(const pp_net& net, long long off, size_t floats) {
    return off >= 0 && (off % 4) == 0 && (size_t)off + floats <= net.n_weights;
}
// the op's parameters: w_floats at w_off and b_floats at b_off (0: the op has no second block, b_off is not looked at)
static int check_params(const pp_net& net, const pp_op& op, int idx, size_t w_floats, size_t b_floats) {
    PP_REQUIRE(blob_holds(net, op.w_off, w_floats) && (b_floats == 0 || blob_holds(net, op.b_off, b_floats)),
               "op %d: %s parameters out of blob (or not 16-byte aligned)", idx, op_kind(op.type).name);
    return PP_OK;
}
static bool buf_is(const pp_net& net, int b, int h, int w, int c) {
    return net.bufs[b].h == h && net.bufs[b].w == w && net.bufs[b].c == c;
}
// an optional residual: absent, or a [h][w][c] buffer that is not the op's out buffer
static int check_res1(const pp_net& net, const pp_op& op, int idx, int h, int w, int c) {
    if (op.res1 >= 0)
        PP_REQUIRE(buf_is(net, op.res1, h, w, c) && op.res1 != op.out, "op %d: %s res1 must be a [%d][%d][%d] buffer other than out", idx,
                   op_kind(op.type).name, h, w, c);
    return PP_OK;
}
// the further coarse terms of the two fuse ops: in3 only behind in2, each [h >> up][w >> up][c] of the out buffer
static int check_coarse_terms(const pp_net& net, const pp_op& op, int idx, int c) {
    const pp_buf& bo = net.bufs[op.out];
    PP_REQUIRE(op.in3 < 0 || op.in2 >= 0, "op %d: in3 without in2", idx);
    for (int k = 0; k < 2; ++k) {
        const int b = k ? op.in3 : op.in2, u = k ? op.up3_log2 : op.up2_log2;
        if (b >= 0)
            PP_REQUIRE(u >= 0 && u <= 5 && net.bufs[b].c == c && (net.bufs[b].h << u) == bo.h && (net.bufs[b].w << u) == bo.w && b != op.out,
                       "op %d: in%d must be [h >> up][w >> up][c] of the out buffer", idx, k + 2);
    }
    return PP_OK;
}
// OpKind::has_no (but for IN2 / IN3, which net_check_op looks at earlier): those fields hold their neutral value
static int check_has_no(const pp_op& op, int idx, const OpKind& kind) {
    const unsigned no = kind.has_no;
    const char* what = (no & RES1) && op.res1 >= 0                    ? "res1"
                       : (no & RES2) && op.res2 >= 0                  ? "res2"
                       : (no & NCHW) && op.out_nchw                   ? "NCHW output"
                       : (no & OUT_SLICE) && op.out_c_off != 0        ? "output slices (out_c_off)"
                       : (no & IN_SLICE) && op.in_c_off != 0          ? "input slices (in_c_off)"
                       : (no & UPSAMPLING) && op.up_log2 != 0         ? "upsampling (up_log2)"
                       : (no & ACTIVATION) && op.relu != PP_RELU_NONE ? "activation"
                                                                      : nullptr;
    PP_REQUIRE(!what, "op %d: %s has no %s", idx, kind.name, what);
    PP_REQUIRE(!(no & ACT_BUT_RELU_LAST) || op.relu == PP_RELU_NONE || op.relu == PP_RELU_LAST, "op %d: %s supports PP_RELU_NONE / PP_RELU_LAST", idx,
               kind.name);
    return PP_OK;
}
#define PP_TRY(expr) do { int _rc = (expr); if (_rc != PP_OK) return _rc; } while (0)

// ---- the op types: check, then launch ---------------------------------------------------------------------------------------------
// PP_OP_CONV
static int check_conv(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    const int eh = op.pad_end & 1, ew = (op.pad_end >> 1) & 1;   // TensorFlow SAME: the odd padding row / column goes last
    PP_REQUIRE(bo.pad == 0 || (!op.out_nchw && op.out_c_off == 0 && bo.c == op.cout && (op.cout & 3) == 0),
               "op %d: a halo output buffer must be a plain NHWC tensor of the op's own channels", idx);
    PP_REQUIRE(bi.c == op.cin && op.in_c_off == 0, "op %d: in buffer has %d channels, op.cin=%d", idx, bi.c, op.cin);
    PP_REQUIRE(op.out_c_off + op.cout <= bo.c && (op.out_c_off == 0 ? true : !op.out_nchw),
               "op %d: channels [%d, %d) do not fit the out buffer (%d channels)", idx, op.out_c_off,
               op.out_c_off + op.cout, bo.c);
    PP_REQUIRE(bo.c == op.cout || ((bo.c & 3) == 0 && !op.out_nchw), "op %d: a sliced out buffer needs c %% 4 == 0", idx);
    PP_REQUIRE(op.relu >= PP_RELU_NONE && op.relu <= PP_ACT_SWISH, "op %d: unknown activation %d", idx, op.relu);
    // bits 2 / 3: padding in front only -- the last output row / column of the symmetric-padding result is not computed
    const int ho = pp_conv_out_dim(bi.h + eh, op.kh, op.stride, op.pad_h, op.dil_h) - ((op.pad_end >> 2) & 1);
    const int wo = pp_conv_out_dim(bi.w + ew, op.kw, op.stride, op.pad_w, op.dil_w) - ((op.pad_end >> 3) & 1);
    PP_REQUIRE((ho << op.up_log2) == bo.h && (wo << op.up_log2) == bo.w,
               "op %d: conv output %dx%d (<<%d) does not match out buffer %dx%d", idx, ho, wo, op.up_log2,
               bo.h, bo.w);
    const size_t kpad = ((size_t)op.kh * op.kw * op.cin + 31) / 32 * 32;
    const size_t cpad = ((size_t)op.cout + 15) / 16 * 16;
    PP_TRY(check_params(net, op, idx, kpad * cpad, cpad));
    if (op.res1 >= 0) PP_REQUIRE(net.bufs[op.res1].c == op.cout, "op %d: res1 channel mismatch", idx);
    if (op.res2 >= 0) PP_REQUIRE(buf_is(net, op.res2, bo.h, bo.w, op.cout), "op %d: res2 shape mismatch", idx);
    return PP_OK;
}
static ConvArgs net_conv_args(pp_net* net, int idx, int batch) {
    const pp_op& op = net->ops[idx];
    const pp_buf &bi = net->bufs[op.in], &bo = net->bufs[op.out];
    ConvArgs a{};
    a.x = net->buf_ptr(op.in);
    a.y = net->buf_ptr(op.out);
    a.w = net->weights + op.w_off;
    a.bias = net->weights + op.b_off;
    a.res1 = net->buf_ptr(op.res1);
    a.res2 = net->buf_ptr(op.res2);
    a.N = batch; a.Hin = bi.h; a.Win = bi.w; a.Cin = op.cin;
    a.Hout = bo.h >> op.up_log2; a.Wout = bo.w >> op.up_log2;
    a.Cout = op.cout; a.CoutPad = (op.cout + 15) / 16 * 16;
    a.KH = op.kh; a.KW = op.kw; a.stride = op.stride; a.pad_h = op.pad_h; a.pad_w = op.pad_w;
    a.dil_h = op.dil_h; a.dil_w = op.dil_w;
    a.K = op.kh * op.kw * op.cin; a.Kpad = (a.K + 31) / 32 * 32;
    a.HWout = a.Hout * a.Wout; a.M = batch * a.HWout;
    a.relu = op.relu; a.up_log2 = op.up_log2; a.out_nchw = op.out_nchw;
    a.res1_shift = op.res1_shift; a.res1_off_w = op.res1_off_w;
    a.res1_H = op.res1 >= 0 ? net->bufs[op.res1].h : 0;
    a.res1_W = op.res1 >= 0 ? net->bufs[op.res1].w : 0;
    a.y_stride = bo.c; a.y_coff = op.out_c_off;
    a.x_pad = bi.pad; a.y_pad = bo.pad;
    a.r1_pad = op.res1 >= 0 ? net->bufs[op.res1].pad : 0;
    a.r2_pad = op.res2 >= 0 ? net->bufs[op.res2].pad : 0;
    // (creation calls this before every plan exists: what is not planned yet is absent)
    const bool planned = (size_t)idx < net->split_plan.size();
    a.wsplit = (net->wsplit && planned && net->split_plan[idx].off >= 0) ? net->wsplit + net->split_plan[idx].off : nullptr;
    a.numerics = net->numerics;
    a.split_f16 = net->split_f16;
    if ((size_t)idx < net->op_x_slot.size()) {
        a.x_amax = net->amax_slot(net->op_x_slot[idx]);
        a.y_amax = net->amax_slot(net->op_y_slot[idx]);
    }
    if (net->carries(idx) >= 0) {      // the folded shortcut: a second K segment in place of res1
        const pp_op& sc = net->ops[net->carries(idx)];
        const pp_buf& bs = net->bufs[sc.in];
        a.res1 = nullptr;
        a.res1_H = a.res1_W = a.r1_pad = 0;
        a.x2 = net->buf_ptr(sc.in);
        a.w2 = net->weights + sc.w_off;
        a.bias2 = net->weights + sc.b_off;
        a.Cin2 = sc.cin; a.Hin2 = bs.h; a.Win2 = bs.w; a.stride2 = sc.stride; a.x2_pad = bs.pad;
        if ((size_t)idx < net->op_x2_slot.size()) a.x2_amax = net->amax_slot(net->op_x2_slot[idx]);
        if (a.wsplit && net->split_plan[idx].cin2 > 0)      // b3 + bs, behind the fragments and scales of the split copy
            a.bias = reinterpret_cast<const float*>(static_cast<const unsigned char*>(a.wsplit) + net->split_plan[idx].bias_off);
    }
    return a;
}
static int launch_conv(pp_net* net, const pp_op&, int idx, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_conv(net_conv_args(net, idx, batch), &net->split_plan[idx], s);
}
static bool conv_fused_amax(pp_net* net, int idx) {
    return pp_conv_tracks_amax(net_conv_args(net, idx, 1), !net->folded(idx) && net->split_plan[idx].kernel != SPLIT_NONE);
}
static bool always(pp_net*, int) { return true; }

// PP_OP_MAXPOOL
static int check_maxpool(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    const int eh = op.pad_end & 1, ew = (op.pad_end >> 1) & 1;
    PP_REQUIRE(op.cin == op.cout && (op.cin & 3) == 0 && op.in_c_off + op.cin <= bi.c && op.out_c_off + op.cout <= bo.c &&
                   (bi.c & 3) == 0 && (bo.c & 3) == 0,
               "op %d: maxpool channel slices do not fit", idx);
    PP_REQUIRE(pp_conv_out_dim(bi.h + eh, op.kh, op.stride, op.pad_h, 1) == bo.h &&
                   pp_conv_out_dim(bi.w + ew, op.kw, op.stride, op.pad_w, 1) == bo.w,
               "op %d: maxpool output dims mismatch", idx);
    return PP_OK;
}
static int launch_maxpool(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    PoolArgs p{};
    p.x = net->buf_ptr(op.in); p.y = net->buf_ptr(op.out);
    p.N = batch; p.Hin = bi.h; p.Win = bi.w; p.C = op.cin; p.Hout = bo.h; p.Wout = bo.w;
    p.x_stride = bi.c; p.x_coff = op.in_c_off; p.y_stride = bo.c; p.y_coff = op.out_c_off;
    p.KH = op.kh; p.KW = op.kw; p.stride = op.stride; p.pad_h = op.pad_h; p.pad_w = op.pad_w;
    return pp_launch_maxpool(p, s);
}

// PP_OP_AVGPOOL
static int check_avgpool(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(op.cin == op.cout && (op.cin & 3) == 0 && bi.c == op.cin && bo.c == op.cin && op.in != op.out && op.kh > 0 &&
                   op.kw > 0 && op.stride > 0 && bi.h >= op.kh && bi.w >= op.kw && (bi.h - op.kh) / op.stride + 1 == bo.h &&
                   (bi.w - op.kw) / op.stride + 1 == bo.w,
               "op %d: avgpool needs in [h][w][c] and out [(h - kh) / s + 1][(w - kw) / s + 1][c], c %% 4 == 0", idx);
    return PP_OK;
}
static int launch_avgpool(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_avgpool(net->buf_ptr(op.in), net->buf_ptr(op.out), batch, bi.h, bi.w, op.cin, op.kh, op.kw, op.stride, s);
}

// PP_OP_COPY
static int check_copy(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(buf_is(net, op.out, bi.h, bi.w, bi.c), "op %d: copy shape mismatch", idx);
    return PP_OK;
}
static int launch_copy(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    PP_HIP_CHECK(hipMemcpyAsync(net->buf_ptr(op.out), net->buf_ptr(op.in), (size_t)batch * net->buf_elems[op.in] * sizeof(float),
                                hipMemcpyDeviceToDevice, s));
    return PP_OK;
}

// PP_OP_DEPTH_TO_SPACE
static int check_depth_to_space(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(op.cout > 0 && (op.cout & 3) == 0 && bi.c == 4 * op.cout && bo.c == op.cout && bo.h == 2 * bi.h && bo.w == 2 * bi.w,
               "op %d: depth_to_space needs in [h][w][4*cout] and out [2h][2w][cout]", idx);
    return PP_OK;
}
static int launch_depth_to_space(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_depth_to_space(net->buf_ptr(op.in), net->buf_ptr(op.out), batch, bi.h, bi.w, op.cout, s);
}

// PP_OP_DECONV_BF16 (its object: pp_net::deconvs, made by pp_net_create_ex)
static int check_deconv_bf16(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(bi.c == op.cin && bo.c == op.cout && bo.h == 2 * bi.h && bo.w == 2 * bi.w && op.in != op.out,
               "op %d: deconv_bf16 needs in [h][w][cin] and out [2h][2w][cout]", idx);
    PP_REQUIRE(op.cin % 64 == 0 && (op.cout & 7) == 0, "op %d: deconv_bf16 needs cin %% 64 == 0 and cout %% 8 == 0", idx);
    return check_params(net, op, idx, (size_t)16 * op.cout * op.cin, op.cout);
}
static int launch_deconv_bf16(pp_net* net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_deconv_bf16_run(net->deconvs[idx], net->buf_ptr(op.in), net->buf_ptr(op.out), batch, op.relu == PP_RELU_LAST, s);
}

// PP_OP_UPSAMPLE_ADD
static int check_upsample_add(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(op.cin == op.cout && (op.cout & 3) == 0 && bi.c == op.cout && bo.c == op.cout && op.up_log2 >= 0 &&
                   (bi.h << op.up_log2) == bo.h && (bi.w << op.up_log2) == bo.w && op.in != op.out,
               "op %d: upsample_add needs in [h][w][c] and out [h << up][w << up][c]", idx);
    for (int r : {op.res1, op.res2})
        if (r >= 0) PP_REQUIRE(buf_is(net, r, bo.h, bo.w, bo.c), "op %d: residual shape mismatch", idx);
    return check_coarse_terms(net, op, idx, bo.c);
}
static int launch_upsample_add(pp_net* net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_upsample_add(net->buf_ptr(op.in), net->buf_ptr(op.res1), net->buf_ptr(op.res2), net->buf_ptr(op.out), batch, bo.h,
                                  bo.w, bo.c, op.up_log2, op.relu == PP_RELU_LAST, s, net->buf_ptr(op.in2), op.up2_log2,
                                  net->buf_ptr(op.in3), op.up3_log2, net->y_amax(idx));
}

// PP_OP_BILINEAR_ADD
static int check_bilinear_add(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(op.cin == op.cout && op.cout > 0 && (op.cout & 3) == 0 && bi.c == op.cout && (bo.c & 3) == 0 &&
                   op.out_c_off + op.cout <= bo.c && op.up_log2 >= 0 && op.up_log2 <= 5 && (bi.h << op.up_log2) == bo.h &&
                   (bi.w << op.up_log2) == bo.w && op.in != op.out,
               "op %d: bilinear_add needs in [h][w][c] and out [h << up][w << up][>= out_c_off + c], c %% 4 == 0", idx);
    PP_TRY(check_res1(net, op, idx, bo.h, bo.w, op.cout));
    return check_coarse_terms(net, op, idx, op.cout);
}
static int launch_bilinear_add(pp_net* net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_bilinear_add(net->buf_ptr(op.in), net->buf_ptr(op.res1), net->buf_ptr(op.out), batch, bo.h, bo.w, op.cout, bo.c,
                                  op.out_c_off, op.up_log2, op.relu == PP_RELU_LAST, s, net->buf_ptr(op.in2), op.up2_log2,
                                  net->buf_ptr(op.in3), op.up3_log2, net->y_amax(idx));
}

// PP_OP_DWCONV3X3
static int check_dwconv3x3(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(op.cin == op.cout && op.cout > 0 && (op.cout & 3) == 0 && bi.c == op.cout && bo.c == op.cout && op.in != op.out,
               "op %d: dwconv3x3 needs distinct in / out buffers of cin == cout channels, a multiple of 4", idx);
    PP_REQUIRE(op.kh == 3 && op.kw == 3 && op.pad_h == 1 && op.pad_w == 1 && (op.stride == 1 || op.stride == 2) &&
                   bo.h == (bi.h - 1) / op.stride + 1 && bo.w == (bi.w - 1) / op.stride + 1,
               "op %d: dwconv3x3 is 3x3, padding 1, stride 1 or 2: in [h][w][c] -> out [(h - 1) / s + 1][(w - 1) / s + 1][c]", idx);
    PP_REQUIRE(op.relu == PP_RELU_NONE || op.relu == PP_RELU_LAST || op.relu == PP_ACT_GELU,
               "op %d: dwconv3x3 supports PP_RELU_NONE / PP_RELU_LAST / PP_ACT_GELU", idx);
    PP_REQUIRE((op.pad_end & ~PP_DW_GELU_IN) == 0 && (!(op.pad_end & PP_DW_GELU_IN) || op.stride == 1),
               "op %d: dwconv3x3 pad_end is 0 or PP_DW_GELU_IN (stride 1 only)", idx);
    return check_params(net, op, idx, (size_t)9 * op.cout, op.cout);
}
static int launch_dwconv3x3(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_dwconv3x3(net->buf_ptr(op.in), net->weights + op.w_off, net->weights + op.b_off, net->buf_ptr(op.out), batch,
                               bi.h, bi.w, op.cout, op.stride, op.relu, op.pad_end & PP_DW_GELU_IN, s);
}

// PP_OP_LAYERNORM
static int check_layernorm(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(op.cin > 0 && op.cin <= op.cout && (op.cout & 3) == 0 && op.cout <= 1024 && bi.c == op.cout && bo.c == op.cout &&
                   bi.h == bo.h && bi.w == bo.w && op.in != op.out,
               "op %d: layernorm needs distinct in / out buffers [h][w][cout], cin <= cout real channels, cout %% 4 == 0, <= 1024", idx);
    return check_params(net, op, idx, op.cout, (size_t)op.cout + 1);
}
static int launch_layernorm(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_layernorm_nhwc(net->buf_ptr(op.in), net->weights + op.w_off, net->weights + op.b_off, net->buf_ptr(op.out),
                                    (size_t)batch * bi.h * bi.w, op.cin, op.cout, s);
}

// PP_OP_WINDOW_ATTN
static int check_window_attn(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(op.stride > 0 && op.cin > 0 && op.cin % op.stride == 0 && op.cin <= op.cout && (op.cout & 3) == 0 &&
                   op.cin / op.stride <= pp_window_attn_max_head_dim(),
               "op %d: window_attn needs cin = heads (stride) * head dim (at most %d) <= cout, cout %% 4 == 0", idx, pp_window_attn_max_head_dim());
    PP_REQUIRE(bi.c == 3 * op.cout && bo.c == op.cout && bi.h == bo.h && bi.w == bo.w && op.in != op.out,
               "op %d: window_attn needs in [h][w][3 * cout] (the qkv map) and out [h][w][cout]", idx);
    PP_REQUIRE(op.kh == 7 && op.kw == 7, "op %d: window_attn supports 7x7 windows", idx);
    return check_params(net, op, idx, (size_t)169 * op.stride, (size_t)3 * op.cout);
}
static int launch_window_attn(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_window_attn(net->buf_ptr(op.in), net->weights + op.w_off, net->weights + op.b_off, net->buf_ptr(op.out), batch,
                                 bi.h, bi.w, op.cin, op.cout, op.stride, s);
}

// PP_OP_ATTENTION
static int check_attention(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(op.stride > 0 && op.cin > 0 && op.cin % op.stride == 0 && op.cin <= op.cout && (op.cout & 3) == 0 &&
                   ((op.cin / op.stride) & 3) == 0 && op.cin / op.stride <= pp_attention_f32_max_head_dim(),
               "op %d: attention needs cin = heads (stride) * head dim (a multiple of 4, at most %d) <= cout, cout %% 4 == 0", idx,
               pp_attention_f32_max_head_dim());
    PP_REQUIRE(bi.c == 3 * op.cout && bo.c == op.cout && bi.h == bo.h && bi.w == bo.w && op.in != op.out &&
                   (long long)bi.h * bi.w <= pp_attention_f32_max_tokens(),
               "op %d: attention needs in [h][w][3 * cout] (the qkv map) and out [h][w][cout], h * w <= %d tokens", idx,
               pp_attention_f32_max_tokens());
    return PP_OK;
}
static int launch_attention(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_attention_f32(net->buf_ptr(op.in), net->buf_ptr(op.out), batch, bi.h * bi.w, op.stride, op.cin, op.cout, s);
}

// PP_OP_GELU_ADD
static int check_gelu_add(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(op.cin == op.cout && op.cout > 0 && (op.cout & 3) == 0 && bi.c == op.cout && bo.c == op.cout && bi.h == bo.h &&
                   bi.w == bo.w && op.in != op.out, "op %d: gelu_add needs distinct in / out buffers [h][w][c], c %% 4 == 0", idx);
    return check_res1(net, op, idx, bo.h, bo.w, bo.c);
}
static int launch_gelu_add(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_gelu_add(net->buf_ptr(op.in), net->buf_ptr(op.res1), net->buf_ptr(op.out), (size_t)batch * net->buf_elems[op.in], s);
}

// PP_OP_DCN3X3 (in2, required: the offset / mask map)
static int check_dcn3x3(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    const pp_buf& bm = net.bufs[op.in2];
    PP_REQUIRE(op.in2 != op.out && op.in != op.out, "op %d: dcn3x3 needs an out buffer distinct from in and in2 (the offset / mask buffer)", idx);
    PP_REQUIRE(op.cin > 0 && (op.cin & 3) == 0 && bi.c == op.cin && op.cout > 0 && op.cout <= pp_dcn3x3_max_cout() && bo.c == op.cout &&
                   bo.h == bi.h && bo.w == bi.w && bm.h == bi.h && bm.w == bi.w && bm.c >= 27,
               "op %d: dcn3x3 needs in [h][w][cin %% 4 == 0], in2 [h][w][>= 27] and out [h][w][cout <= %d]", idx, pp_dcn3x3_max_cout());
    PP_REQUIRE(op.kh == 3 && op.kw == 3 && op.stride == 1 && op.pad_h == 1 && op.pad_w == 1 && op.dil_h == 1 && op.dil_w == 1,
               "op %d: dcn3x3 is 3x3, stride 1, padding 1, dilation 1", idx);
    const size_t cin_p = ((size_t)op.cin + 31) / 32 * 32, cout_p = ((size_t)op.cout + 31) / 32 * 32;
    return check_params(net, op, idx, 9 * cin_p * cout_p, cout_p);
}
static int launch_dcn3x3(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_dcn3x3(net->buf_ptr(op.in), net->buf_ptr(op.in2), net->weights + op.w_off, net->weights + op.b_off,
                            net->buf_ptr(op.out), batch, bi.h, bi.w, op.cin, op.cout, net->bufs[op.in2].c, op.relu == PP_RELU_LAST, s);
}

// PP_OP_DWDECONV
static int check_dwdeconv(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(op.cin == op.cout && op.cout > 0 && (op.cout & 3) == 0 && bi.c == op.cout && bo.c == op.cout && op.in != op.out &&
                   op.stride >= 2 && (op.stride & 1) == 0 && op.kh == 2 * op.stride && op.kw == 2 * op.stride &&
                   op.pad_h == op.stride / 2 && op.pad_w == op.stride / 2 && bo.h == bi.h * op.stride && bo.w == bi.w * op.stride,
               "op %d: dwdeconv needs in [h][w][c] and out [h s][w s][c], c %% 4 == 0, kernel 2 s, padding s / 2, s even", idx);
    PP_TRY(check_res1(net, op, idx, bo.h, bo.w, bo.c));
    return check_params(net, op, idx, (size_t)op.kh * op.kw * op.cout, 0);
}
static int launch_dwdeconv(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_dwdeconv(net->buf_ptr(op.in), net->weights + op.w_off, net->buf_ptr(op.res1), net->buf_ptr(op.out), batch, bi.h,
                              bi.w, op.cout, op.stride, s);
}

// PP_OP_SUB_CAT / PP_OP_BCAST_MUL / PP_OP_BLEND2: one check (in2, blend2: and in3, required), a launch each
static int check_trades_ew(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    const bool cat = op.type == PP_OP_SUB_CAT;
    PP_REQUIRE(op.cin > 0 && (op.cin & 3) == 0 && bi.c == op.cin && op.cout == op.cin + (cat ? 4 : 0) && bo.c == op.cout && bo.h == bi.h &&
                   bo.w == bi.w && op.in != op.out,
               "op %d: needs in [h][w][cin %% 4 == 0] and a distinct out [h][w][cout], cout = cin (sub_cat: cin + 4)", idx);
    PP_REQUIRE((op.type == PP_OP_BCAST_MUL) == (op.res1 < 0), "op %d: sub_cat and blend2 take their second map in res1, bcast_mul takes none", idx);
    PP_TRY(check_res1(net, op, idx, bi.h, bi.w, bi.c));
    for (int b : {op.in2, op.in3})
        if (b >= 0)
            PP_REQUIRE(net.bufs[b].h == bi.h && net.bufs[b].w == bi.w && b != op.out && (cat ? net.bufs[b].c >= 1 && net.bufs[b].c <= 4 : net.bufs[b].c == 1),
                       "op %d: in2 / in3 must be [h][w][1] maps (sub_cat: [h][w][1 .. 4]) other than out", idx);
    return PP_OK;
}
static int launch_sub_cat(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_sub_cat(net->buf_ptr(op.in), net->buf_ptr(op.res1), net->buf_ptr(op.in2), net->buf_ptr(op.out), (size_t)batch * bi.h * bi.w,
                             op.cin, net->bufs[op.in2].c, s);
}
static int launch_bcast_mul(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_bcast_mul(net->buf_ptr(op.in), net->buf_ptr(op.in2), net->buf_ptr(op.out), (size_t)batch * bi.h * bi.w, op.cin, s);
}
static int launch_blend2(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_blend2(net->buf_ptr(op.in), net->buf_ptr(op.res1), net->buf_ptr(op.in2), net->buf_ptr(op.in3), net->buf_ptr(op.out),
                            (size_t)batch * bi.h * bi.w, op.cin, s);
}

// PP_OP_GRAPH_MIX
static int check_graph_mix(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    const int g = op.kh, c = g > 0 ? op.cout / g : 0;
    PP_REQUIRE(g > 0 && g <= 4 && op.cout > 0 && op.cout % g == 0 && (c & 3) == 0 && op.cin == 2 * op.cout && bi.c == op.cin,
               "op %d: graph_mix needs kh = graphs (1 .. 4), cout = graphs * c (c %% 4 == 0) and in [17][w][cin = 2 * cout]", idx);
    PP_REQUIRE(bi.h == 17 && bo.h == 17 && bo.w == bi.w && (bo.c & 3) == 0 && op.out_c_off + op.cout <= bo.c && op.in != op.out,
               "op %d: graph_mix needs in [17][w][cin] and a distinct out [17][w][>= out_c_off + cout], channels %% 4 == 0", idx);
    return check_params(net, op, idx, (size_t)289 * op.cout, (size_t)op.cout + (size_t)17 * g);
}
static int launch_graph_mix(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_graph_mix(net->buf_ptr(op.in), net->weights + op.w_off, net->weights + op.b_off, net->buf_ptr(op.out), batch, bi.h,
                               bi.w, op.kh, op.cout / op.kh, bo.c, op.out_c_off, op.relu == PP_RELU_LAST, s);
}

// PP_OP_JOINT_ATTN
static int check_joint_attn(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(op.stride > 0 && op.cin > 0 && op.cin % op.stride == 0 && op.cin <= op.cout && (op.cout & 3) == 0 &&
                   ((op.cin / op.stride) & 3) == 0 && op.cin / op.stride <= pp_joint_attn_max_head_dim(),
               "op %d: joint_attn needs cin = heads (stride) * head dim (a multiple of 4, at most %d) <= cout, cout %% 4 == 0", idx,
               pp_joint_attn_max_head_dim());
    PP_REQUIRE(bi.h == 17 && bi.c == 3 * op.cout && bo.h == 17 && bo.w == bi.w && (bo.c & 3) == 0 && op.out_c_off + op.cout <= bo.c &&
                   op.in != op.out,
               "op %d: joint_attn needs in [17][w][3 * cout] (the qkv map) and a distinct out [17][w][>= out_c_off + cout]", idx);
    return PP_OK;
}
static int launch_joint_attn(pp_net* net, const pp_op& op, int, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_launch_joint_attn(net->buf_ptr(op.in), net->buf_ptr(op.out), batch, bi.h, bi.w, op.stride, op.cin, op.cout, bo.c,
                                op.out_c_off, s);
}

// PP_OP_VIT_ENCODER (its object: pp_net::vits, made by pp_net_create_ex)
static int check_vit_encoder(const pp_net& net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo) {
    PP_REQUIRE(op.cin == op.cout && bi.c == op.cin && bo.c == op.cin && bi.h == bo.h && bi.w == bo.w && op.in != op.out,
               "op %d: vit encoder needs distinct in / out buffers of [h][w][dim]", idx);
    PP_REQUIRE(op.kh > 0 && op.kw > 0 && op.stride > 0, "op %d: vit encoder needs depth (kh), heads (kw), mlp ratio (stride)", idx);
    return check_params(net, op, idx, pp_vit_param_floats(bi.h * bi.w, op.cin, op.kh, op.cin * op.stride), 0);
}
static int launch_vit_encoder(pp_net* net, const pp_op& op, int idx, const pp_buf& bi, const pp_buf& bo, int batch, hipStream_t s) {
    return pp_vit_encoder_run(net->vits[idx], net->buf_ptr(op.in), net->buf_ptr(op.out), batch, s);
}

static const OpKind& op_kind(int type) {
    static const OpKind none = {nullptr, nullptr, nullptr, IN23, 0, false, nullptr, false};
    static const OpKind kinds[] = {
        /* 0 */ none,
        /* PP_OP_CONV */ {"conv", check_conv, launch_conv, IN23, 0, true, conv_fused_amax, true},
        /* PP_OP_MAXPOOL */ {"maxpool", check_maxpool, launch_maxpool, IN23, 0, false, nullptr, false},
        /* PP_OP_ROIALIGN: the detector's own kernel, no op of a layer program */ none,
        /* PP_OP_COPY */ {"copy", check_copy, launch_copy, IN23, 0, false, nullptr, false},
        /* PP_OP_VIT_ENCODER */ {"vit encoder", check_vit_encoder, launch_vit_encoder, IN23, 0, false, nullptr, false},
        /* PP_OP_DEPTH_TO_SPACE */ {"depth_to_space", check_depth_to_space, launch_depth_to_space, IN23, 0, false, nullptr, false},
        /* PP_OP_UPSAMPLE_ADD */ {"upsample_add", check_upsample_add, launch_upsample_add, ACT_BUT_RELU_LAST, 0, false, always, false},
        /* PP_OP_DECONV_BF16 */ {"deconv_bf16", check_deconv_bf16, launch_deconv_bf16, IN23 | ACT_BUT_RELU_LAST, 0, false, nullptr, false},
        /* PP_OP_AVGPOOL */ {"avgpool", check_avgpool, launch_avgpool, IN23, 0, false, nullptr, false},
        /* PP_OP_BILINEAR_ADD */ {"bilinear_add", check_bilinear_add, launch_bilinear_add, RES2 | NCHW | ACT_BUT_RELU_LAST, 0, false, always, true},
        /* PP_OP_DWCONV3X3 */ {"dwconv3x3", check_dwconv3x3, launch_dwconv3x3, IN23 | RES1 | RES2 | NCHW | OUT_SLICE | UPSAMPLING, 0, false, nullptr, false},
        /* PP_OP_LAYERNORM */ {"layernorm", check_layernorm, launch_layernorm, IN23 | RES1 | RES2 | NCHW | OUT_SLICE, 0, false, nullptr, false},
        /* PP_OP_WINDOW_ATTN */ {"window_attn", check_window_attn, launch_window_attn, IN23 | RES1 | RES2 | NCHW | OUT_SLICE, 0, false, nullptr, false},
        /* PP_OP_GELU_ADD */ {"gelu_add", check_gelu_add, launch_gelu_add, IN23 | RES2 | NCHW | OUT_SLICE, 0, false, nullptr, false},
        /* PP_OP_ATTENTION */ {"attention", check_attention, launch_attention, IN23 | RES1 | RES2 | NCHW | OUT_SLICE, 0, false, nullptr, false},
        /* PP_OP_DCN3X3 */ {"dcn3x3", check_dcn3x3, launch_dcn3x3, IN3 | RES1 | RES2 | NCHW | OUT_SLICE | UPSAMPLING | ACT_BUT_RELU_LAST, IN2, false, nullptr, false},
        /* PP_OP_DWDECONV */ {"dwdeconv", check_dwdeconv, launch_dwdeconv, IN23 | RES2 | NCHW | OUT_SLICE | UPSAMPLING | ACTIVATION, 0, false, nullptr, false},
        /* PP_OP_SUB_CAT */ {"sub_cat", check_trades_ew, launch_sub_cat, IN3 | RES2 | NCHW | OUT_SLICE | IN_SLICE | UPSAMPLING | ACTIVATION, IN2, false, nullptr, false},
        /* PP_OP_BCAST_MUL */ {"bcast_mul", check_trades_ew, launch_bcast_mul, IN3 | RES2 | NCHW | OUT_SLICE | IN_SLICE | UPSAMPLING | ACTIVATION, IN2, false, nullptr, false},
        /* PP_OP_BLEND2 */ {"blend2", check_trades_ew, launch_blend2, RES2 | NCHW | OUT_SLICE | IN_SLICE | UPSAMPLING | ACTIVATION, IN23, false, nullptr, false},
        /* PP_OP_GRAPH_MIX */ {"graph_mix", check_graph_mix, launch_graph_mix, IN23 | RES1 | RES2 | NCHW | IN_SLICE | UPSAMPLING | ACT_BUT_RELU_LAST, 0, false, nullptr, false},
        /* PP_OP_JOINT_ATTN */ {"joint_attn", check_joint_attn, launch_joint_attn, IN23 | RES1 | RES2 | NCHW | IN_SLICE | UPSAMPLING | ACTIVATION, 0, false, nullptr, false},
    };
    static_assert(sizeof(kinds) / sizeof(kinds[0]) == PP_OP_JOINT_ATTN + 1, "one row per op type, in the order of the PP_OP_* constants");
    return type >= 0 && type < (int)(sizeof(kinds) / sizeof(kinds[0])) ? kinds[type] : none;
}

// what holds for every op type, from the table; then the type's own check
static int net_check_op(const pp_net& net, const pp_op& op, int idx) {
    const int nb = (int)net.bufs.size();
    const OpKind& kind = op_kind(op.type);
    const char* name = kind.name ? kind.name : "this op type";
    PP_REQUIRE(op.in >= 0 && op.in < nb && op.out >= 0 && op.out < nb, "op %d: buffer id out of range", idx);
    PP_REQUIRE(op.res1 < nb && op.res2 < nb, "op %d: residual buffer id out of range", idx);
    PP_REQUIRE(op.in2 < nb && op.in3 < nb && (op.in2 < 0 || !(kind.has_no & IN2)) && (op.in3 < 0 || !(kind.has_no & IN3)),
               "op %d: %s does not take in%d, or its buffer id is out of range (in2 / in3 are -1 where an op type has no such input)", idx, name,
               op.in2 >= nb || (op.in2 >= 0 && (kind.has_no & IN2)) ? 2 : 3);
    PP_REQUIRE(op.out_c_off >= 0 && op.in_c_off >= 0 && (op.out_c_off & 3) == 0 && (op.in_c_off & 3) == 0,
               "op %d: channel offsets must be non-negative multiples of 4", idx);
    if (!kind.halo)
        for (int b : {op.in, op.out, op.res1, op.res2, op.in2, op.in3})
            PP_REQUIRE(b < 0 || net.bufs[b].pad == 0, "op %d: only convolutions may touch a buffer with a zero halo (buffer %d)", idx, b);
    if (!kind.check) {
        pp_set_error("op %d: unsupported op type %d", idx, op.type);
        return PP_ERR_UNSUPPORTED;
    }
    PP_REQUIRE((!(kind.needs & IN2) || op.in2 >= 0) && (!(kind.needs & IN3) || op.in3 >= 0), "op %d: %s needs in%d", idx, name,
               (kind.needs & IN2) && op.in2 < 0 ? 2 : 3);
    PP_TRY(check_has_no(op, idx, kind));
    return kind.check(net, op, idx, net.bufs[op.in], net.bufs[op.out]);
}

static int net_launch_op(pp_net* net, int idx, int batch, hipStream_t s) {
    if (net->folded(idx)) return PP_OK;      // a folded shortcut: computed inside the op that carries it
    const pp_op& op = net->ops[idx];
    int rc = op_kind(op.type).launch(net, op, idx, net->bufs[op.in], net->bufs[op.out], batch, s);
    if (rc == PP_OK && net->amax && net->op_post_slot[idx] >= 0)
        rc = pp_launch_amax(net->buf_ptr(op.out), batch, net->buf_elems[op.out], net->amax_slot(net->op_post_slot[idx]), s);
    return rc;
}

// layer classes whose shortcut is NOT folded: "<B's cin>+<A's cin>" or "...@<out h>x<out w>", comma-separated (pp_net_folded_into).
// The built-in list holds the classes that measured no faster folded (DESIGN_LOG.md, "Folded projection shortcuts")
static const char* const kFoldOffBuiltin = "";
static bool fold_class_on(int cin_b, int cin_a, int h, int w) {
    const char* env = getenv("POSEPIPE_SPLIT_FOLD_OFF");
    const std::string list = std::string(",") + (env ? env : kFoldOffBuiltin) + ",";
    char key[64];
    snprintf(key, sizeof(key), ",%d+%d,", cin_b, cin_a);
    if (list.find(key) != std::string::npos) return false;
    snprintf(key, sizeof(key), ",%d+%d@%dx%d,", cin_b, cin_a, h, w);
    return list.find(key) == std::string::npos;
}

// Projection shortcuts of ResNet-style bottlenecks: act(W3 h + b3 + (Ws x + bs)) as ONE product over the concatenated K (see
// conv_split_gemm_kernel, SEG2) -- the shortcut tensor is neither written nor read back and its launch disappears.  Pattern:
//   A: 1x1 convolution (any stride, no padding), no activation, no residuals, a plain NHWC tensor of its own;
//   A's output is read by exactly one op B before the buffer is overwritten (or the program ends), only as B's res1 with
//   res1_shift == 0, and nobody writes A's INPUT between A and B (B reads it in A's place);
//   B: 1x1 / stride-1 convolution that the split plan puts on the product kernel in the fp16 form; same output geometry as A.
// Runs after every op has its plan and before the maxima and lanes are planned: both see the dataflow as executed (pp_net::reads).
static void net_fold_shortcuts(pp_net* net) {
    const int n = (int)net->ops.size();
    net->fold_into.assign(n, -1);
    net->fold_src.assign(n, -1);
    const char* env = getenv("POSEPIPE_SPLIT_FOLD");
    if (net->numerics != PP_NET_NUMERICS_SPLIT || !net->split_f16 || (env && atoi(env) == 0)) return;
    for (int ia = 0; ia < n; ++ia) {
        const pp_op& A = net->ops[ia];
        if (A.type != PP_OP_CONV || A.kh != 1 || A.kw != 1 || A.pad_h != 0 || A.pad_w != 0 || A.pad_end != 0 || A.stride < 1 ||
            A.relu != PP_RELU_NONE || A.res1 >= 0 || A.res2 >= 0 || A.up_log2 != 0 || A.out_nchw || A.out_c_off != 0 || A.in == A.out ||
            net->bufs[A.out].c != A.cout || net->bufs[A.out].pad != 0 || net->bufs[A.in].pad != 0 || A.cin % 16 != 0 || net->carries(ia) >= 0)
            continue;
        // the readers of A's tensor, and what happens to A's input meanwhile
        int ib = -1, nread = 0;
        bool ok = true;
        for (int j = ia + 1; j < n && ok; ++j) {
            const pp_op& o = net->ops[j];
            int uses = 0;
            for (int b : {o.in, o.res1, o.res2, o.in2, o.in3}) uses += b == A.out;
            if (uses) {
                ++nread;
                ib = j;
                ok = nread == 1 && uses == 1 && o.res1 == A.out;
            }
            if (o.out == A.out) break;                    // the buffer holds another tensor from here on
            if (nread == 0 && o.out == A.in) ok = false;  // A's input changes before B would read it
        }
        if (!ok || nread != 1) continue;
        const pp_op& B = net->ops[ib];
        const pp_buf &ya = net->bufs[A.out], &yb = net->bufs[B.out];
        if (B.type != PP_OP_CONV || B.kh != 1 || B.kw != 1 || B.stride != 1 || B.res1_shift != 0 || B.res1_off_w != 0 || B.up_log2 != 0 ||
            B.cout != A.cout || yb.h != ya.h || yb.w != ya.w || B.out == A.in || net->carries(ib) >= 0 || net->folded(ib) ||
            net->split_plan[ib].kernel != SPLIT_PRODUCT || !net->split_plan[ib].f16 || !fold_class_on(B.cin, A.cin, yb.h, yb.w))
            continue;
        net->fold_into[ia] = ib;
        net->fold_src[ib] = ia;
        const SplitPlan p = pp_conv_split_plan(net_conv_args(net, ib, 1));
        if (p.kernel != SPLIT_PRODUCT || p.cin2 != A.cin) {      // the product kernel does not take this pair: two launches, as before
            net->fold_into[ia] = net->fold_src[ib] = -1;
            continue;
        }
        net->split_plan[ib] = p;
        net->split_plan[ia] = SplitPlan();
    }
}

int pp_net_dims(pp_net* net, int buf, int* h, int* w, int* c) {
    if (!net || buf < 0 || buf >= (int)net->bufs.size()) return PP_ERR_ARG;
    *h = net->bufs[buf].h; *w = net->bufs[buf].w; *c = net->bufs[buf].c;
    return PP_OK;
}
int pp_net_max_batch(pp_net* net) { return net ? net->max_batch : 0; }
pp_ctx* pp_net_ctx(pp_net* net) { return net ? net->ctx : nullptr; }
// the resident weight blob (device pointer) and its length in floats
const float* pp_net_weights(pp_net* net, size_t* n_weights) {
    if (n_weights) *n_weights = net ? net->n_weights : 0;
    return net ? net->weights : nullptr;
}

// the caller's own kernel has just overwritten `buf`: a pending promise of its maxima (pp_net_input_amax) is void
void pp_net_void_input_amax(pp_net* net, int buf) {
    if (!net) return;
    for (auto& e : net->ext)
        if (e.buf == buf) e.provided = false;
}

unsigned* pp_net_input_amax_slot(pp_net* net, int buf) {
    if (!net || !net->amax) return nullptr;
    for (auto& e : net->ext)
        if (e.buf == buf) return net->amax_slot(e.slot);
    return nullptr;
}

extern "C" {

int pp_net_create(pp_ctx* ctx, const pp_op* ops, int n_ops, const pp_buf* bufs, int n_bufs,
                  const float* weights, size_t n_weights, int max_batch, pp_net** out) {
    return pp_net_create_mem(ctx, ops, n_ops, bufs, n_bufs, weights, n_weights, PP_MEM_HOST, max_batch, out);
}

int pp_net_create_mem(pp_ctx* ctx, const pp_op* ops, int n_ops, const pp_buf* bufs, int n_bufs,
                      const float* weights, size_t n_weights, int weights_mem, int max_batch, pp_net** out) {
    return pp_net_create_ex(ctx, ops, n_ops, bufs, n_bufs, weights, n_weights, weights_mem, max_batch, PP_NET_NUMERICS_DEFAULT, out);
}

int pp_net_numerics(pp_net* net) { return net ? net->numerics : PP_ERR_ARG; }
int pp_net_split_kind(pp_net* net) {
    if (!net) return PP_ERR_ARG;
    return net->numerics != PP_NET_NUMERICS_SPLIT ? PP_NET_NUMERICS_EXACT : net->split_f16 ? PP_NET_NUMERICS_SPLIT_F16 : PP_NET_NUMERICS_SPLIT_BF16;
}

// The net lives in a unique_ptr until the last line: every early return below (PP_REQUIRE, PP_HIP_CHECK, a failed step's code)
// releases what was built so far through ~pp_net.
int pp_net_create_ex(pp_ctx* ctx, const pp_op* ops, int n_ops, const pp_buf* bufs, int n_bufs,
                     const float* weights, size_t n_weights, int weights_mem, int max_batch, int numerics, pp_net** out) {
    PP_REQUIRE(ctx && ops && bufs && weights && out, "pp_net_create: NULL argument");
    PP_REQUIRE(numerics >= PP_NET_NUMERICS_DEFAULT && numerics <= PP_NET_NUMERICS_SPLIT_F16, "pp_net_create_ex: bad numerics %d", numerics);
    PP_REQUIRE(weights_mem == PP_MEM_HOST || weights_mem == PP_MEM_DEVICE, "pp_net_create: bad weights_mem %d", weights_mem);
    PP_REQUIRE(n_ops > 0 && n_bufs > 0 && max_batch > 0, "pp_net_create: empty program");
    *out = nullptr;
    std::unique_ptr<pp_net> net(new pp_net());
    net->ctx = ctx;
    net->ops.assign(ops, ops + n_ops);
    net->bufs.assign(bufs, bufs + n_bufs);
    net->max_batch = max_batch;
    net->n_weights = n_weights;
    // the process-wide switch is read HERE, once: later pp_conv_exact calls (or other threads) do not change this net
    net->numerics = numerics != PP_NET_NUMERICS_DEFAULT ? numerics : (pp_conv_split_enabled() ? PP_NET_NUMERICS_SPLIT : PP_NET_NUMERICS_EXACT);
    if (net->numerics >= PP_NET_NUMERICS_SPLIT) {       // the split form: named, or the process-wide default at this moment
        net->split_f16 = net->numerics == PP_NET_NUMERICS_SPLIT ? pp_conv_split_f16_default() : net->numerics == PP_NET_NUMERICS_SPLIT_F16;
        net->numerics = PP_NET_NUMERICS_SPLIT;
    }
    size_t off = 0;
    for (int b = 0; b < n_bufs; ++b) {
        PP_REQUIRE(bufs[b].h > 0 && bufs[b].w > 0 && bufs[b].c > 0 && bufs[b].pad >= 0 && bufs[b].pad <= 8, "buffer %d has an empty dim / bad halo", b);
        const size_t e = (size_t)(bufs[b].h + bufs[b].pad) * (bufs[b].w + bufs[b].pad) * bufs[b].c;   // halo: never written, stays zero
        net->buf_elems.push_back(e);
        net->buf_off.push_back(off);
        off += (e * max_batch + 63) / 64 * 64;   // 256-byte aligned
    }
    net->arena_floats = off;
    for (int i = 0; i < n_ops; ++i) PP_TRY(net_check_op(*net, net->ops[i], i));
    PP_HIP_CHECK(hipSetDevice(ctx->device));
    PP_HIP_CHECK(hipMalloc((void**)&net->weights, n_weights * sizeof(float)));
    PP_HIP_CHECK(hipMemcpyAsync(net->weights, weights, n_weights * sizeof(float),
                                weights_mem == PP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
    PP_HIP_CHECK(hipMalloc((void**)&net->arena, net->arena_floats * sizeof(float)));
    PP_HIP_CHECK(hipMemsetAsync(net->arena, 0, net->arena_floats * sizeof(float), ctx->stream));
    net->vits.assign(n_ops, nullptr);
    net->deconvs.assign(n_ops, nullptr);
    for (int i = 0; i < n_ops; ++i) {
        const pp_op& op = net->ops[i];
        const pp_buf& bi = net->bufs[op.in];
        if (op.type == PP_OP_DECONV_BF16)
            PP_TRY(pp_deconv_bf16_create(net->weights + op.w_off, net->weights + op.b_off, bi.h, bi.w, op.cin, op.cout, max_batch,
                                         ctx->stream, &net->deconvs[i]));
        if (op.type == PP_OP_VIT_ENCODER)
            PP_TRY(pp_vit_encoder_create(net->weights + op.w_off, bi.h * bi.w, op.cin, op.kh, op.kw, op.cin * op.stride, max_batch,
                                         ctx->stream, &net->vits[i]));
    }
    // each conv op's split kernel, planned once, and the bf16-split copies of the weights of every conv it will run
    net->split_plan.assign(n_ops, SplitPlan());
    if (net->numerics == PP_NET_NUMERICS_SPLIT) {
        size_t bytes = 0;
        for (int i = 0; i < n_ops; ++i) {
            if (net->ops[i].type != PP_OP_CONV) continue;
            SplitPlan p = pp_conv_split_plan(net_conv_args(net.get(), i, 1));
            if (p.kernel == SPLIT_NONE) continue;
            net->split_plan[i] = p;
        }
        net_fold_shortcuts(net.get());
        for (int i = 0; i < n_ops; ++i) {
            SplitPlan& p = net->split_plan[i];
            if (p.kernel == SPLIT_NONE) continue;
            p.off = (long long)bytes;
            bytes += (p.bytes + 255) / 256 * 256;
        }
        net_plan_amax(net.get());
        if (!net->slot_owner.empty()) {
            const size_t ab = net->slot_owner.size() * (size_t)max_batch * sizeof(unsigned);
            PP_HIP_CHECK(hipMalloc((void**)&net->amax, ab));
            PP_HIP_CHECK(hipMemsetAsync(net->amax, 0, ab, ctx->stream));
        }
        if (bytes) {
            PP_HIP_CHECK(hipMalloc((void**)&net->wsplit, bytes));
            for (int i = 0; i < n_ops; ++i) {
                const SplitPlan& p = net->split_plan[i];
                if (p.kernel == SPLIT_NONE) continue;
                ConvArgs ca = net_conv_args(net.get(), i, 1);
                ca.bias = net->weights + net->ops[i].b_off;      // (a folded op: its own bias -- the sum is made from it here)
                PP_TRY(pp_conv_split_weights(p, ca, net->wsplit + p.off, ctx->stream));
            }
        }
    }
    PP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    // per-geometry tables of the pipelined conv kernel: built here, never inside a launch that may be under graph capture
    for (int i = 0; i < n_ops; ++i)
        if (net->ops[i].type == PP_OP_CONV) PP_TRY(pp_conv_prepare(net_conv_args(net.get(), i, 1)));
    const char* env_lanes = getenv("POSEPIPE_NET_LANES");
    PP_TRY(net_make_lanes(net.get(), env_lanes ? atoi(env_lanes) : 4));
    *out = net.release();
    return PP_OK;
}

// (re)build the lane streams, the op -> lane plan and its events for `n_lanes` (<= 1, or a program under 8 ops: none -- every op on the
// ctx stream).  The caller has synchronised: nothing of the net is in flight.
static int net_make_lanes(pp_net* net, int n_lanes) {
    net->drop_lanes();
    const int n_ops = (int)net->ops.size();
    if (n_lanes > 1 && n_ops >= 8) {
        net_plan_lanes(net, n_lanes);
        net->lanes.resize(n_lanes);
        for (auto& l : net->lanes) PP_HIP_CHECK(hipStreamCreateWithFlags(&l, hipStreamNonBlocking));
        net->op_done.assign(n_ops, nullptr);
        for (int i = 0; i < n_ops; ++i)
            if (net->op_needs_event[i]) PP_HIP_CHECK(hipEventCreateWithFlags(&net->op_done[i], hipEventDisableTiming));
        PP_HIP_CHECK(hipEventCreateWithFlags(&net->fork_ev, hipEventDisableTiming));
        net->join_ev.resize(n_lanes);
        for (auto& e : net->join_ev) PP_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    return PP_OK;
}

int pp_net_input_amax(pp_net* net, int buf, void** dptr) {
    PP_REQUIRE(net && dptr && buf >= 0 && buf < (int)net->bufs.size(), "pp_net_input_amax: bad argument");
    *dptr = nullptr;
    for (auto& e : net->ext)
        if (e.buf == buf && net->amax) {
            e.provided = true;
            *dptr = net->amax_slot(e.slot);
        }
    return PP_OK;
}

int pp_net_conv_kinds(pp_net* net, int* kinds) {
    PP_REQUIRE(net && kinds, "pp_net_conv_kinds: NULL argument");
    for (size_t i = 0; i < net->ops.size(); ++i) {
        // (a folded shortcut keeps kind 2: its product runs on the split kernel, inside the op that carries it -- so sums of a caller's
        // per-op FLOPs by kind stay whole; pp_net_profile reports it with 0 ms and pp_net_folded_into names the carrying op)
        kinds[i] = net->ops[i].type != PP_OP_CONV ? 0 : net->split_plan[i].kernel != SPLIT_NONE || net->folded((int)i) ? 2 : 1;
    }
    return PP_OK;
}

int pp_net_folded_into(pp_net* net, int* into) {
    PP_REQUIRE(net && into, "pp_net_folded_into: NULL argument");
    for (size_t i = 0; i < net->ops.size(); ++i) into[i] = net->folded((int)i) ? net->fold_into[i] : -1;
    return PP_OK;
}

void pp_net_destroy(pp_net* net) { delete net; }      // ~pp_net: synchronises first

int pp_net_buffer(pp_net* net, int buf, void** dptr, size_t* bytes_per_sample) {
    PP_REQUIRE(net && buf >= 0 && buf < (int)net->bufs.size(), "pp_net_buffer: bad buffer id");
    PP_REQUIRE(net->bufs[buf].pad == 0, "pp_net_buffer: buffer %d has a zero halo (conv-internal layout); expose dense buffers only", buf);
    if (dptr) *dptr = net->buf_ptr(buf);
    if (bytes_per_sample) *bytes_per_sample = net->buf_elems[buf] * sizeof(float);
    return PP_OK;
}

int pp_net_run(pp_net* net, int batch, int first_op, int last_op) {
    PP_REQUIRE(net, "pp_net_run: net is NULL");
    PP_REQUIRE(batch > 0 && batch <= net->max_batch, "pp_net_run: batch %d not in (0,%d]", batch, net->max_batch);
    if (last_op < 0) last_op = (int)net->ops.size();
    PP_REQUIRE(first_op >= 0 && last_op <= (int)net->ops.size() && first_op <= last_op, "pp_net_run: bad op range");
    if (net->graph_exec && batch == net->graph_batch && first_op == 0 && last_op == (int)net->ops.size()) {
        PP_HIP_CHECK(hipGraphLaunch(net->graph_exec, net->ctx->stream));
        // the replay is the run a pending promise (pp_net_input_amax) covered: whether the graph takes the maxima itself was fixed at
        // capture, and a promise left standing would make the next eager run skip its maxima pass and scale by stale maxima
        for (auto& e : net->ext) e.provided = false;
        return PP_OK;
    }
    hipStream_t main = net->ctx->stream;
    PpRange range("pp_net_run");
    PP_TRY(net_reset_amax(net, first_op, last_op, batch, main));
    if (net->lanes.empty() || !net->use_lanes || last_op - first_op < 8) {
        for (int i = first_op; i < last_op; ++i) PP_TRY(net_launch_op(net, i, batch, main));
        return PP_OK;
    }
    // fork: every lane starts after whatever is already queued on the ctx stream
    PP_HIP_CHECK(hipEventRecord(net->fork_ev, main));
    for (hipStream_t l : net->lanes) PP_HIP_CHECK(hipStreamWaitEvent(l, net->fork_ev, 0));
    for (int i = first_op; i < last_op; ++i) {
        hipStream_t s = net->lanes[net->op_lane[i]];
        for (int d : net->op_waits[i])
            if (d >= first_op) PP_HIP_CHECK(hipStreamWaitEvent(s, net->op_done[d], 0));
        PP_TRY(net_launch_op(net, i, batch, s));
        if (net->op_needs_event[i]) PP_HIP_CHECK(hipEventRecord(net->op_done[i], s));
    }
    // join: the ctx stream continues after every lane
    for (size_t l = 0; l < net->lanes.size(); ++l) {
        PP_HIP_CHECK(hipEventRecord(net->join_ev[l], net->lanes[l]));
        PP_HIP_CHECK(hipStreamWaitEvent(main, net->join_ev[l], 0));
    }
    return PP_OK;
}

int pp_net_vit_timing(pp_net* net, int enable, float* ms3, int* n_gemm) {
    PP_REQUIRE(net, "pp_net_vit_timing: net is NULL");
    for (auto* v : net->vits) {
        if (!v) continue;
        if (ms3) {
            PP_HIP_CHECK(hipStreamSynchronize(net->ctx->stream));
            PP_TRY(pp_vit_encoder_get_timing(v, ms3, n_gemm));
        }
        pp_vit_encoder_set_timing(v, enable);
        return PP_OK;
    }
    pp_set_error("pp_net_vit_timing: the program has no PP_OP_VIT_ENCODER");
    return PP_ERR_STATE;
}

int pp_net_set_lane_count(pp_net* net, int n_lanes) {
    PP_REQUIRE(net && n_lanes >= 1 && n_lanes <= 16, "pp_net_set_lane_count: net is NULL or n_lanes not in [1, 16]");
    PP_HIP_CHECK(hipStreamSynchronize(net->ctx->stream));
    for (auto l : net->lanes) PP_HIP_CHECK(hipStreamSynchronize(l));
    if (net->graph_exec) {            // a captured graph holds the old plan
        PP_HIP_CHECK(hipGraphExecDestroy(net->graph_exec));
        net->graph_exec = nullptr;
    }
    return net_make_lanes(net, n_lanes);
}

int pp_net_set_lanes(pp_net* net, int enable) {
    PP_REQUIRE(net, "pp_net_set_lanes: net is NULL");
    PP_HIP_CHECK(hipStreamSynchronize(net->ctx->stream));
    net->use_lanes = enable != 0;
    return PP_OK;
}

int pp_net_capture(pp_net* net, int batch) {
    PP_REQUIRE(net, "pp_net_capture: net is NULL");
    PP_REQUIRE(batch > 0 && batch <= net->max_batch, "pp_net_capture: bad batch");
    if (net->graph_exec) {
        PP_HIP_CHECK(hipGraphExecDestroy(net->graph_exec));
        net->graph_exec = nullptr;
    }
    hipStream_t s = net->ctx->stream;
    PP_HIP_CHECK(hipStreamSynchronize(s));
    hipGraph_t graph = nullptr;
    PP_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc = net_reset_amax(net, 0, (int)net->ops.size(), batch, s);
    for (int i = 0; i < (int)net->ops.size() && rc == PP_OK; ++i) rc = net_launch_op(net, i, batch, s);
    hipError_t e = hipStreamEndCapture(s, &graph);
    if (rc != PP_OK) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }
    PP_HIP_CHECK(e);
    PP_HIP_CHECK(hipGraphInstantiate(&net->graph_exec, graph, nullptr, nullptr, 0));
    PP_HIP_CHECK(hipGraphDestroy(graph));
    net->graph_batch = batch;
    return PP_OK;
}

int pp_net_forward(pp_net* net, int batch, int in_buf, const float* in, int out_buf, float* out, int mem) {
    PP_REQUIRE(net && in && out, "pp_net_forward: NULL argument");
    PP_REQUIRE(in_buf >= 0 && in_buf < (int)net->bufs.size() && out_buf >= 0 && out_buf < (int)net->bufs.size(),
               "pp_net_forward: bad buffer id");
    PP_REQUIRE(batch > 0 && batch <= net->max_batch, "pp_net_forward: batch %d not in (0,%d]", batch, net->max_batch);
    PP_REQUIRE(net->bufs[in_buf].pad == 0 && net->bufs[out_buf].pad == 0, "pp_net_forward: input / output buffers must be dense (pad 0)");
    hipStream_t s = net->ctx->stream;
    const hipMemcpyKind kin = mem == PP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    const hipMemcpyKind kout = mem == PP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    PP_HIP_CHECK(hipMemcpyAsync(net->buf_ptr(in_buf), in, (size_t)batch * net->buf_elems[in_buf] * sizeof(float), kin, s));
    pp_net_void_input_amax(net, in_buf);      // the input was just overwritten here
    PP_TRY(pp_net_run(net, batch, 0, (int)net->ops.size()));
    PP_HIP_CHECK(hipMemcpyAsync(out, net->buf_ptr(out_buf), (size_t)batch * net->buf_elems[out_buf] * sizeof(float), kout, s));
    PP_HIP_CHECK(hipStreamSynchronize(s));
    return PP_OK;
}

int pp_net_profile(pp_net* net, int batch, float* ms_per_op) {
    PP_REQUIRE(net, "pp_net_profile: net is NULL");
    PP_REQUIRE(batch > 0 && batch <= net->max_batch, "pp_net_profile: bad batch");
    hipStream_t s = net->ctx->stream;
    const int n = (int)net->ops.size();
    std::vector<hipEvent_t> ev(n + 1, nullptr);
    auto timed_run = [&]() -> int {
        for (auto& e : ev) PP_HIP_CHECK(hipEventCreate(&e));
        int rc = net_reset_amax(net, 0, n, batch, s);
        PP_HIP_CHECK(hipEventRecord(ev[0], s));
        for (int i = 0; i < n && rc == PP_OK; ++i) {
            rc = net_launch_op(net, i, batch, s);
            if (rc == PP_OK && hipEventRecord(ev[i + 1], s) != hipSuccess) rc = PP_ERR_HIP;
        }
        if (rc == PP_OK && hipStreamSynchronize(s) != hipSuccess) rc = PP_ERR_HIP;
        return rc;
    };
    const int rc = timed_run();
    if (rc == PP_OK && ms_per_op) {
        for (int i = 0; i < n; ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            ms_per_op[i] = ms;
        }
    }
    for (auto e : ev)      // on every way out of the run
        if (e) (void)hipEventDestroy(e);
    return rc;
}

}  // extern "C"
