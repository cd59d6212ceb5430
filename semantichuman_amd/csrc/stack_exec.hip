// Whole-stack execution (sh_stack_forward / sh_stack_backward): host-side sequencing of the conv / spmm /
// activation-backward / weight-gradient entry points for one encoder or decoder stack.  It mirrors, launch for
// launch, what semantichuman_amd/stack.py does call by call from Python (reference: the layer loops of
// models.py:119-128 and :146-153 plus autograd's backward chain) - the point is host time: one call instead of
// ~25 us of interpreter and ctypes work per launch.  No kernels here.
#include "sh_common.h"

namespace {

struct Lay { long sv, sb; };                                   // element strides of (row, batch)
inline Lay lay(int layout, int rows, int B, int C) {
    return layout == 0 ? Lay{(long)B * C, (long)C} : Lay{(long)C, (long)rows * C};
}
inline int out_rows(const sh_stack_step& s) { return s.kind == 0 ? s.R : s.m_rows; }
inline bool is_last_step(int i, int n) { return i == n - 1; }
inline int in_rows(const sh_stack_step& s) { return s.kind == 0 ? s.n_in : s.m_cols; }

// Every tensor a step gathers from is addressed with 32-bit offsets: element offsets in the fp32 conv kernels, row offsets
// pre-multiplied by the row stride in 16-byte units in the plane convs (csrc/p3_conv.hip: tv[]) and the streaming weight
// gradients (Tl[]).  2^32 ELEMENTS per tensor is the tightest of the three (16 GiB of fp32, 24 GiB of planes against the 64 GiB
// the pre-multiplied forms reach), so that is what is refused here - with a message, not with wrapped gather addresses.
int check_tensor_sizes(int n, const sh_stack_step* st, int rows0, int c0, int B, const char* what) {
    long rows = rows0;
    int c = c0;
    for (int i = 0; i <= n; ++i) {
        long extra = 0;                                       // pre-summed rows behind a conv step's gradient rows
        if (i > 0 && st[i - 1].kind == 0) extra = (long)st[i - 1].n1 + st[i - 1].n2;
        SH_REQUIRE((rows + extra) * (long)B * c < (1L << 32), SH_ERR_UNSUPPORTED,
                   "%s: the tensor %s step %d has %ld rows x %d batch entries x %d channels >= 2^32 elements - split the batch", what,
                   i < n ? "entering" : "leaving", i < n ? i : n - 1, rows + extra, B, c);
        if (i == n) break;
        rows = st[i].kind == 0 ? st[i].R : (st[i].extend ? (long)st[i].m_cols + st[i].m_rows : st[i].m_rows);
        if (st[i].kind == 0) c = st[i].cout;
    }
    return SH_OK;
}

int check_steps(int n, const sh_stack_step* st, int c0, const char* what) {
    SH_REQUIRE(n > 0 && st, SH_ERR_INVALID_ARG, "%s: no steps", what);
    int c = c0;
    for (int i = 0; i < n; ++i) {
        SH_REQUIRE(st[i].kind == 0 || st[i].kind == 1, SH_ERR_INVALID_ARG, "%s: step %d has kind %d", what, i, st[i].kind);
        if (st[i].kind == 0) {
            SH_REQUIRE(st[i].cin == c, SH_ERR_INVALID_ARG, "%s: step %d takes %d channels, its input has %d", what, i, st[i].cin, c);
            SH_REQUIRE(st[i].table && st[i].param >= 0, SH_ERR_INVALID_ARG, "%s: step %d incomplete", what, i);
            c = st[i].cout;
        } else {
            SH_REQUIRE(st[i].m.rowptr && st[i].m.col && st[i].m.val, SH_ERR_INVALID_ARG, "%s: step %d has no matrix", what, i);
        }
    }
    return SH_OK;
}

// What every sequencer checks first; `what` is the entry point's name, `pointers` whether its required pointers are all there.
int check_call(int n, const sh_stack_step* st, int rows0, int c0, int B, bool pointers, const char* what) {
    int rc = check_steps(n, st, c0, what);
    if (rc != SH_OK) return rc;
    if (B > 0 && (rc = check_tensor_sizes(n, st, rows0, c0, B, what)) != SH_OK) return rc;
    SH_REQUIRE(pointers && B > 0, SH_ERR_INVALID_ARG, "%s: null pointer or empty batch", what);
    SH_REQUIRE(n <= 64, SH_ERR_UNSUPPORTED, "%s: more than 64 steps", what);
    return SH_OK;
}

// channels entering step i
void fill_cin_of(int n, const sh_stack_step* st, int c0, int* cin_of) {
    for (int i = 0, c = c0; i < n; ++i) { cin_of[i] = c; if (st[i].kind == 0) c = st[i].cout; }
}

// bf16 path: the fragment-ordered working copies of the conv weights (transpose: the backward-data operands; skip_first: not of step
// 0, whose input gradient nobody wants) - every conv step has its buffer, and ONE launch fills them unless the caller did (ready)
int prep_wfrags(int n_steps, const sh_stack_step* steps, const float* const* weights, void* const* frag, int transpose, bool skip_first,
                bool ready, const char* what, sh_stream_t stream) {
    const float* w[64]; void* wf[64]; int S[64], Ci[64], Co[64], tr[64];
    int n = 0;
    for (int i = skip_first ? 1 : 0; i < n_steps; ++i) {
        if (steps[i].kind != 0) continue;
        SH_REQUIRE(frag && frag[i], SH_ERR_INVALID_ARG, "%s: no weight-fragment buffer for step %d", what, i);
        w[n] = weights[steps[i].param]; wf[n] = frag[i]; S[n] = steps[i].S; Ci[n] = steps[i].cin; Co[n] = steps[i].cout; tr[n] = transpose;
        ++n;
    }
    return n && !ready ? sh_conv_wfrag_prep_multi(n, w, wf, S, Ci, Co, tr, stream) : SH_OK;
}

// The reductions of the weight-gradient slabs, deferred to the end of a backward pass: 16 layers per launch.
struct ReduceJobs {
    typedef int (*Reduce)(int, const void* const*, float* const*, float* const*, const int*, const int*, const int*, const int*, const int*,
                          const int*, sh_stream_t);
    const void* ws[64]; float* dW[64]; float* db[64]; int B[64], R[64], S[64], Ci[64], Co[64], kind[64];
    int n = 0;
    void add(const void* workspace, float* dw, float* dbias, int b, const sh_stack_step& s, int k) {
        ws[n] = workspace; dW[n] = dw; db[n] = dbias; B[n] = b; R[n] = s.R; S[n] = s.S; Ci[n] = s.cin; Co[n] = s.cout; kind[n] = k;
        ++n;
    }
    int flush(Reduce reduce, sh_stream_t stream) const {
        for (int k = 0; k < n; k += 16) {
            const int rc = reduce(n - k < 16 ? n - k : 16, ws + k, dW + k, db + k, B + k, R + k, S + k, Ci + k, Co + k, kind + k, stream);
            if (rc != SH_OK) return rc;
        }
        return SH_OK;
    }
};
int reduce_bf16(int n, const void* const* ws, float* const* dW, float* const* db, const int* B, const int* R, const int* S, const int* Ci,
                const int* Co, const int*, sh_stream_t stream) {
    return sh_spiral_conv_bwd_wgt_reduce_multi_bf16(n, ws, dW, db, B, R, S, Ci, Co, stream);
}

// ---- The kernel forms of an fp32 stack (sh_stack_plan_f32).  plan_f32 decides, for every step and both passes, which kernels run:
// from the steps, the batch, the input layout, whether the three-plane form (SH_MMA_PLANES3) is on, keep_fp32 and the switches
// below.  sh_stack_forward and sh_stack_backward compute the same plan and only carry it out, so the backward pass reads a forward
// image exactly where the forward pass wrote one and leaves unread exactly the fp32 rows the forward pass left unwritten.  Buffers
// follow the plan (a per-step pointer the plan needs and the caller left NULL is an error); two things stay outside it: a frozen
// layer (dW[p] == NULL drops what lives in the weight-gradient launch) and the size of the caller's workspace.
// the switches, read once ("Switches": each has a reader outside the library): SH_P3_N16_MAXB (the rule in plan_f32);
// SH_P3_WGRAD, SH_P3_DROP_FP32, SH_P3_RAGGED, SH_P3_GROUPED = 0: that plane form off (with SH_P3_WGRAD=0 the backward pass reads no
// forward image)
struct Switches { int n16_maxb, wgrad, drop_fp32, ragged, grouped; };
const Switches& switches() {
    static const Switches s{sh_env_int("SH_P3_N16_MAXB", 256, 0, 1 << 30), sh_env_int("SH_P3_WGRAD", 1, 0, 1), sh_env_int("SH_P3_DROP_FP32", 1, 0, 1),
                            sh_env_int("SH_P3_RAGGED", 1, 0, 1), sh_env_int("SH_P3_GROUPED", 1, 0, 1)};
    return s;
}

enum { BD_F32 = 0, BD_TABLE, BD_RAG, BD_GRP };      // backward-data: fp32 kernels; plane kernel over table_t / ragged / grouped lists
struct Forms {
    // forward
    bool f_p3;              // conv: the plane kernel, on the image of its input (sh_spiral_conv_fwd_p3)
    bool f_grp;             // ... over grouped lists (sh_spiral_conv_p3_grp)
    bool f_img;             // the step writes the image of its output, because the conv that gathers it takes f_p3
    bool f_img_only;        // ... and leaves the fp32 rows unwritten
    // backward, for a trained layer
    bool b_gimg;            // the step's pre-activation gradient gets an image (gin_planes[i + 1] / dpre_last_planes)
    bool b_thin;            // role-swapped weight gradient, which computes the input gradient too (wgrad_thin.hip)
    int b_data;             // backward-data form (BD_*) wherever b_thin does not run (a frozen layer)
    bool b_ride;            // the last pre-sum level rides in the weight-gradient launch
    bool b_presum_img;      // the pre-summed rows get an image (else the plane kernel splits them from the fp32 rows)
    bool b_p3w;             // weight gradient from the two images (wgrad_p3.hip)
    bool b_yimg;            // the plane backward-data kernel takes the activation derivative from the forward image
    bool b_in_img_only;     // keep_fp32 == 2: the fp32 rows of the step's input may be unwritten - the step must run on images
    bool b_grad_img_only;   // keep_fp32 == 2: its pre-activation gradient is handed over as the image alone
};

// the conv step that gathers the buffer step i writes (through a folded up-sampling that appends to it), or -1
inline int consumer_conv(int n, const sh_stack_step* st, int i) {
    int j = i + 1;
    if (j < n && st[j].kind == 1 && st[j].extend) ++j;
    return (j < n && st[j].kind == 0) ? j : -1;
}

void plan_f32(int n, const sh_stack_step* st, int B, int x_layout, bool planes3, int keep_fp32, bool need_x_grad, Forms* f) {
    const Switches& sw = switches();
    for (int i = 0; i < n; ++i) f[i] = Forms{};
    for (int i = 1; i < n && planes3; ++i) {
        const sh_stack_step& s = st[i];
        if (s.kind != 0) continue;
        // the kernels' shape test, and one measured rule: a layer with <= 16 output channels (one channel tile: 6 MFMAs per gathered 3-KiB
        // fragment) loses to the exact staged kernel once the batch is large - per 64 meshes, dec3 (6891 rows, K = 320 -> 16): plane
        // 50.6 / 58.1 / 63.4 / 65.4 / 67.9 us at batch 64 / 128 / 256 / 512 / 1024, exact 68.8 / 66.6 / 63.4 / 60.4 / 56.5
        // (profiles/r05_decode_batch_sweep.txt)
        f[i].f_p3 = !(s.cout <= 16 && B > sw.n16_maxb) && sh_spiral_conv_p3_ok(B, s.S, s.cin, s.cout);
        // grouped lists (round 6): output rows with overlapping spirals share one list of the union - every row gathered once
        f[i].f_grp = f[i].f_p3 && sw.grouped && s.fg_rows && s.fg_pos && s.fg_out && s.fg_n > 0 &&
                     sh_spiral_conv_p3_grp_ok(B, s.S, s.cin, s.cout, s.fg_L) && sh_spiral_conv_p3_grp_pays(B, s.fg_n);
    }
    for (int i = 0; i + 1 < n; ++i) {
        const int c = consumer_conv(n, st, i);
        f[i].f_img = c >= 0 && f[c].f_p3;
    }
    for (int i = 0; i < n; ++i) {
        const sh_stack_step& s = st[i];
        Forms& q = f[i];
        if (s.kind != 0 || !(i > 0 || need_x_grad) || !s.table_t) continue;
        // backward-data on the image of the pre-activation gradient where the kernels take the transposed shape
        q.b_gimg = planes3 && sh_spiral_conv_p3_ok(B, s.S, s.cout, s.cin);
        // a 16 -> 3 channel layer takes its weight gradient in role-swapped form (wgrad_thin.hip), on a plain vertex-major input
        q.b_thin = s.R == s.n_in && (i > 0 || x_layout == 0) && sh_spiral_conv_bwd_wgt_thin_ok(B, s.n_in, s.S, s.cin, s.cout, SH_DTYPE_F32);
        if (q.b_gimg) {
            // ragged source lists (round 6): every source an image row, no pre-summed rows - neither the launches that fill them nor the
            // rider; as GROUPS of input rows sharing one list where the launch has groups enough (also the layers that gather 16
            // channels, which the one-row list kernel does not take)
            const bool grp = sw.ragged && sw.grouped && s.bg_rows && s.bg_pos && s.bg_out && s.bg_n > 0 &&
                             sh_spiral_conv_p3_grp_ok(B, s.S, s.cout, s.cin, s.bg_L) && sh_spiral_conv_p3_grp_pays(B, s.bg_n);
            const bool rag = sw.ragged && s.rag_rows && s.rag_pos && sh_spiral_conv_p3_rag_ok(B, s.S, s.cout, s.cin, s.rag_L);
            q.b_data = grp ? BD_GRP : rag ? BD_RAG : BD_TABLE;
            // pre-summed rows: imaged by their producers (the riders / pre-sum launches), or - LDS-resident plane kernel and at least
            // half as many of them as real rows - left fp32 and split by the backward-data kernel itself (they are ~6 % of what it
            // gathers; the riders' image stores cost their hosts more)
            q.b_presum_img = !(sh_spiral_conv_p3_kind(B, s.S, s.cout, s.cin) == 1 && 2 * (s.n1 + s.n2) >= s.R);
        }
        const bool p3 = q.b_data != BD_F32 && !q.b_thin;
        q.b_ride = !q.b_thin && q.b_data < BD_RAG && (s.n1 || s.n2);
        // the weight gradient from the two images: the image of the step's input exists (the forward pass wrote it) and the kernel
        // takes the shape
        q.b_p3w = p3 && sw.wgrad && i > 0 && f[i - 1].f_img && sh_spiral_conv_bwd_wgt_p3_ok(B, s.R, s.S, s.cin, s.cout) &&
                  (((long)s.R * (B / 16)) % 2 == 0 || s.zero_row >= 0);
        q.b_yimg = q.b_data != BD_F32 && sw.wgrad && i > 0 && st[i - 1].kind == 0 && f[i - 1].f_img;
        q.b_in_img_only = keep_fp32 == 2 && sw.drop_fp32 && q.b_p3w;
        // ... and its gradient rows, when besides no pre-sum launch or rider reads them: list forms, or a table without multiplicities
        q.b_grad_img_only = q.b_in_img_only && (q.b_data >= BD_RAG || (s.n1 == 0 && s.n2 == 0));
    }
    // forward only (keep_fp32 == 0), or training on the images where the backward pass of the consumer leaves them unread too
    // (keep_fp32 == 2): rows that are gathered through their plane image alone are written as the image alone - a re-sampling step in
    // front of a plane conv, a plane conv directly in front of another (through a folded up-sampling its fp32 rows feed the blend)
    for (int i = 0; i + 1 < n; ++i) {
        const int c = consumer_conv(n, st, i);
        f[i].f_img_only = f[i].f_img && (keep_fp32 == 0 || f[c].b_in_img_only) && (st[i].kind == 1 || (f[i].f_p3 && c == i + 1));
    }
}

}  // namespace

extern "C" {

int sh_stack_plan_f32(int n_steps, const sh_stack_step* steps, int c0, int B, int x_layout, int mma_mode, int keep_fp32, int need_x_grad,
                      int* forms) {
    int rc = check_steps(n_steps, steps, c0, "sh_stack_plan_f32");
    if (rc != SH_OK) return rc;
    SH_REQUIRE(forms && B > 0 && n_steps <= 64 && sh_mma_mode_valid(mma_mode) && keep_fp32 >= 0 && keep_fp32 <= 2, SH_ERR_INVALID_ARG,
               "sh_stack_plan_f32: null pointer, empty batch, more than 64 steps, mma_mode %d or keep_fp32 %d", mma_mode, keep_fp32);
    Forms f[64];
    plan_f32(n_steps, steps, B, x_layout, mma_mode == SH_MMA_PLANES3, keep_fp32, need_x_grad != 0, f);
    for (int i = 0; i < n_steps; ++i) {
        const Forms& q = f[i];
        const int bd = q.b_thin ? BD_F32 : q.b_data;
        const bool on[15] = {q.f_p3, q.f_grp, q.f_img, q.f_img_only, q.b_gimg, q.b_thin, bd != BD_F32, bd == BD_RAG, bd == BD_GRP, q.b_ride,
                             bd != BD_F32 && q.b_presum_img, q.b_p3w, q.b_yimg, q.b_in_img_only, q.b_grad_img_only};      // enum sh_stack_form
        forms[i] = 0;
        for (int k = 0; k < 15; ++k) forms[i] |= on[k] ? 1 << k : 0;
    }
    return SH_OK;
}

int sh_stack_forward(int n_steps, const sh_stack_step* steps, const float* x, int x_layout, int rows0, int c0, int B,
                     const float* const* weights, const float* const* biases, float* const* outs, int out_layout, int mma_mode,
                     void* const* planes, const void* const* wfrag3, int keep_fp32, sh_stream_t stream) {
    int rc = check_call(n_steps, steps, rows0, c0, B, x && weights && outs, "sh_stack_forward");
    if (rc != SH_OK) return rc;
    SH_REQUIRE(sh_mma_mode_valid(mma_mode), SH_ERR_INVALID_ARG, "sh_stack_forward: unknown mma_mode %d", mma_mode);
    SH_REQUIRE(keep_fp32 >= 0 && keep_fp32 <= 2, SH_ERR_INVALID_ARG, "sh_stack_forward: keep_fp32 = %d (0, 1 or 2)", keep_fp32);
    Forms f[64];
    plan_f32(n_steps, steps, B, x_layout, mma_mode == SH_MMA_PLANES3 && planes && wfrag3, keep_fp32, false, f);
    for (int i = 0; i < n_steps; ++i) {
        SH_REQUIRE(outs[i], SH_ERR_INVALID_ARG, "sh_stack_forward: no output buffer for step %d", i);
        SH_REQUIRE(!f[i].f_img || planes[i], SH_ERR_INVALID_ARG, "sh_stack_forward: step %d writes the image of its output: planes[%d] is NULL", i, i);
        SH_REQUIRE(!f[i].f_p3 || wfrag3[i], SH_ERR_INVALID_ARG, "sh_stack_forward: step %d runs on planes: wfrag3[%d] is NULL", i, i);
    }
    const float* cur = x;
    Lay cl = lay(x_layout, rows0, B, c0);
    int c = c0;
    for (int i = 0; i < n_steps; ++i) {
        const sh_stack_step& s = steps[i];
        const Forms& q = f[i];
        const int co = s.kind == 0 ? s.cout : c;
        const Lay ol = lay(i == n_steps - 1 ? out_layout : 0, out_rows(s), B, co);
        void* img = q.f_img ? planes[i] : nullptr;
        if (s.kind == 0) {
            const float* bias = biases ? biases[s.param] : nullptr;
            float* y = q.f_img_only ? nullptr : outs[i];
            if (q.f_grp)
                rc = sh_spiral_conv_p3_grp(planes[i - 1], s.fg_rows, s.fg_pos, s.fg_out, s.fg_n, s.fg_L, wfrag3[i], bias, y, ol.sv, ol.sb, img, nullptr,
                                           0, 0, nullptr, s.act, s.zero_row, 0, B, s.R, s.S, s.cin, s.cout, stream);
            else if (q.f_p3)
                rc = sh_spiral_conv_fwd_p3(planes[i - 1], s.table, wfrag3[i], bias, y, ol.sv, ol.sb, img, B, s.R, s.S, s.cin, s.cout, s.act,
                                           s.zero_row, stream);
            else
                rc = sh_spiral_conv_fwd_img(cur, cl.sv, cl.sb, s.table, weights[s.param], bias, outs[i], ol.sv, ol.sb, img, B, s.R, s.S, s.cin,
                                            s.cout, s.act, s.zero_row, mma_mode, stream);
        } else if (s.extend) {
            SH_REQUIRE(i > 0 && !is_last_step(i, n_steps) && outs[i] == outs[i - 1] && cl.sb == c, SH_ERR_INVALID_ARG,
                       "sh_stack_forward: step %d appends to its input, which must be the vertex-major output buffer of step %d", i, i - 1);
            SH_REQUIRE(!img || planes[i] == planes[i - 1], SH_ERR_INVALID_ARG, "sh_stack_forward: step %d appends to its input: same image buffer", i);
            float* dst = q.f_img_only ? nullptr : outs[i] + (long)s.m_cols * cl.sv;
            rc = sh_spmm_p3(s.m.rowptr, s.m.col, s.m.val, cur, cl.sv, cl.sb, dst, cl.sv, cl.sb,
                            img ? static_cast<char*>(img) + sh_p3_bytes(s.m_cols, B, c) : nullptr, nullptr, 0, 0, 0, -1, B, s.m_rows, c, stream);
        } else {
            rc = sh_spmm_p3(s.m.rowptr, s.m.col, s.m.val, cur, cl.sv, cl.sb, q.f_img_only ? nullptr : outs[i], ol.sv, ol.sb, img, nullptr, 0, 0, 0,
                            -1, B, s.m_rows, c, stream);
        }
        if (rc != SH_OK) return rc;
        cur = outs[i]; cl = ol; c = co;
    }
    return SH_OK;
}

int sh_stack_backward(int n_steps, const sh_stack_step* steps, const float* x, int x_layout, int rows0, int c0, int B,
                      const float* const* acts, const float* g, int out_layout, const float* const* weights,
                      float* const* gin, float* dpre_last, float* const* weight_t, void* const* workspace,
                      const size_t* workspace_bytes, float* const* dW, float* const* dbias, int need_x_grad, int mma_mode,
                      void* const* gin_planes, void* dpre_last_planes, const void* const* wfrag3_t, const void* const* in_planes,
                      int acts_fp32, sh_stream_t stream) {
    int rc = check_call(n_steps, steps, rows0, c0, B, x && acts && g && weights && gin && dW, "sh_stack_backward");
    if (rc != SH_OK) return rc;
    SH_REQUIRE(sh_mma_mode_valid(mma_mode), SH_ERR_INVALID_ARG, "sh_stack_backward: unknown mma_mode %d", mma_mode);
    const bool planes3 = mma_mode == SH_MMA_PLANES3 && gin_planes && wfrag3_t;
    SH_REQUIRE(acts_fp32 == 1 || (acts_fp32 == 2 && planes3 && in_planes), SH_ERR_INVALID_ARG,
               "sh_stack_backward: acts_fp32 = %d (1: every activation has its fp32 rows; 2, three-plane form with gin_planes, wfrag3_t and "
               "in_planes: the forward pass ran with keep_fp32 == 2)", acts_fp32);
    const int last = n_steps - 1;
    Forms f[64];
    plan_f32(n_steps, steps, B, x_layout, planes3, acts_fp32, need_x_grad != 0, f);
    for (int i = 0; i < n_steps; ++i) {
        SH_REQUIRE(!f[i].b_gimg || (wfrag3_t[i] && (i == last ? dpre_last_planes : gin_planes[i + 1])), SH_ERR_INVALID_ARG,
                   "sh_stack_backward: step %d runs backward-data on planes: wfrag3_t[%d] and the image buffer of its gradient (%s) are required",
                   i, i, i == last ? "dpre_last_planes" : "gin_planes[i + 1]");
        SH_REQUIRE(!in_planes || !(f[i].b_p3w || f[i].b_yimg) || in_planes[i], SH_ERR_INVALID_ARG,
                   "sh_stack_backward: step %d reads the image of its input: in_planes[%d] is NULL", i, i);
    }
    int cin_of[64];
    fill_cin_of(n_steps, steps, c0, cin_of);
    // all weight transposes of the stack (backward-data on planes reads fragments instead): workgroups of the launch that opens the
    // pass (the last step's activation backward), or a launch of their own when the pass opens with a re-sampling step
    const float* tr_w[32]; float* tr_wt[32]; int tr_S[32], tr_Ci[32], tr_Co[32];
    int n_tr = 0;
    for (int i = 0; i < n_steps; ++i) {
        if (steps[i].kind != 0 || !(i > 0 || need_x_grad) || (f[i].b_gimg && !f[i].b_thin)) continue;
        SH_REQUIRE(weight_t && weight_t[i], SH_ERR_INVALID_ARG, "sh_stack_backward: no weight_t buffer for step %d", i);
        SH_REQUIRE(n_tr < 32, SH_ERR_UNSUPPORTED, "sh_stack_backward: more than 32 conv steps");
        tr_w[n_tr] = weights[steps[i].param]; tr_wt[n_tr] = weight_t[i]; tr_S[n_tr] = steps[i].S; tr_Ci[n_tr] = steps[i].cin; tr_Co[n_tr] = steps[i].cout;
        ++n_tr;
    }
    if (n_tr && steps[last].kind != 0) {
        rc = sh_weight_transpose_multi(n_tr, tr_w, tr_wt, tr_S, tr_Ci, tr_Co, stream);
        if (rc != SH_OK) return rc;
        n_tr = 0;
    }
    // gradient entering the last step
    const float* cur; Lay cl;
    void* cur_img = nullptr;                                   // image buffer of `cur` when its consumer gathers planes
    bool cur_img_done = false;                                 // rows [0, R) of it already written by the producer
    {
        const sh_stack_step& s = steps[last];
        if (s.kind == 0) {
            SH_REQUIRE(dpre_last, SH_ERR_INVALID_ARG, "sh_stack_backward: no dpre_last buffer");
            const Lay ol = lay(out_layout, s.R, B, s.cout), dl = lay(0, 0, B, s.cout);
            cur_img = f[last].b_gimg ? dpre_last_planes : nullptr;
            // the image of dpre rides in the launch when that is the plain element-wise form (16-byte quads, no tile turning)
            const bool img_in = cur_img && s.cout % 4 == 0 && s.cout > 8;
            rc = sh_act_backward_tr_img(g, ol.sv, ol.sb, acts[last], ol.sv, ol.sb, dpre_last, dl.sv, dl.sb, img_in ? cur_img : nullptr, B, s.R,
                                        s.cout, s.act, s.zero_row, n_tr, tr_w, tr_wt, tr_S, tr_Ci, tr_Co, stream);
            if (rc != SH_OK) return rc;
            cur = dpre_last; cl = dl;
            cur_img_done = img_in;
        } else {
            cur = g; cl = lay(out_layout, s.m_rows, B, cin_of[last]);
        }
    }
    ReduceJobs jobs;
    for (int i = last; i >= 0; --i) {
        const sh_stack_step& s = steps[i];
        const Forms& q = f[i];
        const bool want_in = i > 0 || need_x_grad;
        const float* inp = i == 0 ? x : acts[i - 1];
        const Lay il = i == 0 ? lay(x_layout, rows0, B, c0) : lay(0, 0, B, cin_of[i]);
        float* gi = want_in ? gin[i] : nullptr;
        SH_REQUIRE(!want_in || gi, SH_ERR_INVALID_ARG, "sh_stack_backward: no gradient buffer for the input of step %d", i);
        const Lay gl = il;
        // the activation derivative of the layer that produced this step's input is applied by whoever writes gin[i]
        const float* yprev = nullptr; Lay yl{0, 0}; int act_prev = 0, zero_prev = -1;
        if (i > 0 && steps[i - 1].kind == 0) {
            yprev = acts[i - 1]; yl = lay(0, 0, B, steps[i - 1].cout); act_prev = steps[i - 1].act; zero_prev = steps[i - 1].zero_row;
        }
        // gin[i] is the pre-activation gradient of conv step i - 1: its image when that step's backward-data pass gathers planes;
        // written as the image alone when that step reads nothing else (acts_fp32 == 2)
        void* gi_img = (i > 0 && steps[i - 1].kind == 0 && f[i - 1].b_gimg) ? gin_planes[i] : nullptr;
        float* gi_f = (gi_img && f[i - 1].b_grad_img_only) ? nullptr : gi;
        bool gi_img_done = false;
        if (s.kind == 0) {
            SH_REQUIRE(workspace && workspace[i], SH_ERR_INVALID_ARG, "sh_stack_backward: no workspace for step %d", i);
            // dW[param] == NULL: a frozen layer - no weight gradient; what rides in that launch (the last pre-sum level, the thin
            // layer's input gradient) runs in the launches the step takes without it
            const bool wgrad = dW[s.param] != nullptr;
            SH_REQUIRE(wgrad || !dbias || !dbias[s.param], SH_ERR_INVALID_ARG,
                       "sh_stack_backward: parameter %d has a dbias buffer but no dW buffer", s.param);
            // the role-swapped weight gradient reads the extended gradient buffer through the transposed table, so it runs after the
            // pre-sum launches below
            const bool thin = wgrad && q.b_thin;
            const int bd = thin ? BD_F32 : q.b_data;
            const bool p3 = bd != BD_F32, rag = bd >= BD_RAG;
            const bool ride = wgrad && q.b_ride;
            char* pimg0 = (p3 && q.b_presum_img) ? static_cast<char*>(cur_img) : nullptr;
            float* mut0 = const_cast<float*>(cur);
            if (ride && s.n1 && s.n2) {
                rc = sh_spmm_p3(s.sum1.rowptr, s.sum1.col, s.sum1.val, cur, cl.sv, cl.sb, mut0 + (long)s.R * cl.sv, cl.sv, cl.sb,
                                pimg0 ? pimg0 + sh_p3_bytes(s.R, B, s.cout) : nullptr, nullptr, 0, 0, 0, -1, B, s.n1, s.cout, stream);
                if (rc != SH_OK) return rc;
            }
            const bool p3w = wgrad && q.b_p3w && in_planes && workspace_bytes[i] >= sh_spiral_conv_bwd_wgt_p3_workspace(B, s.R, s.S, s.cin, s.cout);
            SH_REQUIRE(!q.b_in_img_only || p3w, SH_ERR_INVALID_ARG,
                       "sh_stack_backward: step %d: the forward pass kept only the image of its input (keep_fp32 == 2) but this pass cannot run "
                       "the step on images (a frozen layer, or a workspace smaller than sh_spiral_conv_bwd_wgt_p3_workspace)", i);
            if (wgrad && !thin) {
                const sh_csr_ref& lm = s.n2 ? s.sum2 : s.sum1;
                const int ln = ride ? (s.n2 ? s.n2 : s.n1) : 0;
                float* lout = mut0 + (long)(s.R + (s.n2 ? s.n1 : 0)) * cl.sv;
                void* limg = (ln && pimg0) ? pimg0 + sh_p3_bytes(s.R + (s.n2 ? s.n1 : 0), B, s.cout) : nullptr;
                if (p3w) {
                    if (!cur_img_done) {                       // the gradient rows' image, unless their producer wrote it
                        rc = sh_to_p3(cur, cl.sv, cl.sb, cur_img, B, s.R, s.cout, stream);
                        if (rc != SH_OK) return rc;
                        cur_img_done = true;
                    }
                    rc = sh_spiral_conv_bwd_wgt_p3_presum(cur_img, s.zero_row, in_planes[i], s.table, workspace[i], workspace_bytes[i], cur, cl.sv, cl.sb,
                                                          ln ? lm.rowptr : nullptr, ln ? lm.col : nullptr, ln ? lm.val : nullptr,
                                                          ln ? lout : nullptr, limg, ln, B, s.R, s.S, s.cin, s.cout, stream);
                } else {
                    rc = sh_spiral_conv_bwd_wgt_presum(cur, cl.sv, cl.sb, inp, il.sv, il.sb, s.table, nullptr, nullptr, workspace[i],
                                                       workspace_bytes[i], ln ? lm.rowptr : nullptr, ln ? lm.col : nullptr,
                                                       ln ? lm.val : nullptr, ln ? lout : nullptr, limg, ln, B, s.R, s.S, s.cin, s.cout, mma_mode,
                                                       stream);
                }
                if (rc != SH_OK) return rc;
            }
            if (wgrad) jobs.add(workspace[i], dW[s.param], dbias ? dbias[s.param] : nullptr, B, s, p3w ? 2 : 0);
            if (want_in) {
                SH_REQUIRE(s.table_t, SH_ERR_INVALID_ARG, "sh_stack_backward: step %d has no transposed table", i);
                float* mut = const_cast<float*>(cur);          // the extra rows behind the R real ones of this step's own buffer
                char* pimg = pimg0;
                if (s.n1 && !ride && !rag) {
                    rc = sh_spmm_p3(s.sum1.rowptr, s.sum1.col, s.sum1.val, cur, cl.sv, cl.sb, mut + (long)s.R * cl.sv, cl.sv, cl.sb,
                                    pimg ? pimg + sh_p3_bytes(s.R, B, s.cout) : nullptr, nullptr, 0, 0, 0, -1, B, s.n1, s.cout, stream);
                    if (rc != SH_OK) return rc;
                }
                if (s.n2 && !ride && !rag) {
                    rc = sh_spmm_p3(s.sum2.rowptr, s.sum2.col, s.sum2.val, cur, cl.sv, cl.sb, mut + (long)(s.R + s.n1) * cl.sv,
                                    cl.sv, cl.sb, pimg ? pimg + sh_p3_bytes(s.R + s.n1, B, s.cout) : nullptr, nullptr, 0, 0, 0, -1, B, s.n2,
                                    s.cout, stream);
                    if (rc != SH_OK) return rc;
                }
                if (thin) {
                    // ... and computes the input gradient from the same staged gradient rows
                    rc = sh_spiral_conv_bwd_wgt_thin(cur, cl.sv, cl.sb, inp, SH_DTYPE_F32, il.sv, il.sb, s.table_t, workspace[i],
                                                     workspace_bytes[i], weights[s.param], gi, gl.sv, gl.sb, gi_img, yprev ? act_prev : SH_ACT_IDENTITY,
                                                     zero_prev, B, s.R, s.n_in, s.S, s.cin, s.cout, SH_DTYPE_F32, stream);
                    gi_img_done = gi_img != nullptr;
                } else if (p3) {
                    // image of the gradient rows this pass gathers: the R real rows unless their producer wrote them (the pre-sum
                    // launches wrote the image of their rows)
                    if (!cur_img_done) {
                        rc = sh_to_p3(cur, cl.sv, cl.sb, cur_img, B, s.R, s.cout, stream);
                        if (rc != SH_OK) return rc;
                    }
                    // the activation to differentiate, from its image when the plan says so (SH_P3_YPREV_IMG=0: fp32)
                    const void* yimg = (q.b_yimg && in_planes) ? in_planes[i] : nullptr;
                    if (bd == BD_GRP)
                        rc = sh_spiral_conv_p3_grp(cur_img, s.bg_rows, s.bg_pos, s.bg_out, s.bg_n, s.bg_L, wfrag3_t[i], nullptr, gi_f, gl.sv, gl.sb,
                                                   gi_img, yprev, yl.sv, yl.sb, yimg, act_prev, zero_prev, 1, B, s.n_in, s.S, s.cout, s.cin, stream);
                    else if (bd == BD_RAG)
                        rc = sh_spiral_conv_bwd_data_p3_rag(cur_img, s.rag_rows, s.rag_pos, s.rag_L, wfrag3_t[i], gi_f, gl.sv, gl.sb, gi_img, yprev,
                                                            yl.sv, yl.sb, yimg, act_prev, zero_prev, B, s.n_in, s.S, s.cin, s.cout, stream);
                    else
                        rc = sh_spiral_conv_bwd_data_p3(cur_img, s.zero_row, q.b_presum_img ? nullptr : cur, cl.sv, cl.sb, s.R, s.table_t, wfrag3_t[i],
                                                        gi_f, gl.sv, gl.sb, gi_img, yprev, yl.sv, yl.sb, yimg, act_prev, zero_prev, B, s.n_in, s.S,
                                                        s.cin, s.cout, stream);
                    gi_img_done = gi_img != nullptr;
                } else {
                    // the "no source" entries of table_t point at this step's own dummy row of dpre (stack.py ConvStep.finalize),
                    // which its producer forced to zero
                    rc = sh_spiral_conv_bwd_data_z(cur, cl.sv, cl.sb, s.zero_row, s.table_t, weight_t[i], gi, gl.sv, gl.sb, yprev, yl.sv,
                                                   yl.sb, act_prev, zero_prev, B, s.n_in, s.S, s.cin, s.cout, mma_mode, stream);
                }
                if (rc != SH_OK) return rc;
            }
        } else if (want_in) {
            SH_REQUIRE(s.mt.rowptr && s.mt.col && s.mt.val, SH_ERR_INVALID_ARG, "sh_stack_backward: step %d has no transposed matrix", i);
            rc = sh_spmm_p3(s.mt.rowptr, s.mt.col, s.mt.val, cur, cl.sv, cl.sb, gi_f, gl.sv, gl.sb, gi_img, yprev, yl.sv, yl.sb,
                            act_prev, zero_prev, B, s.m_cols, cin_of[i], stream);
            if (rc != SH_OK) return rc;
            gi_img_done = gi_img != nullptr;
        }
        if (want_in) { cur = gi; cl = gl; cur_img = gi_img; cur_img_done = gi_img_done; }
    }
    return jobs.flush(sh_spiral_conv_bwd_wgt_reduce_multi_kinds, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// The same two sequencers for the bf16 compute path (BASELINE config 3).  Tensors between steps are bf16 vertex-major;
// the stack input may be fp32 with 3 channels (xyz), the stack output fp32 when it has <= 16 channels (x_hat).  The
// working copies of the conv weights are converted from the fp32 masters by ONE launch at the start of each pass.
static inline long esz_of(int dtype) { return dtype == SH_DTYPE_BF16 ? 2 : 4; }

int sh_stack_forward_bf16(int n_steps, const sh_stack_step* steps, const void* x, int x_dtype, int x_layout, int rows0, int c0, int B,
                          const float* const* weights, const float* const* biases, void* const* wfrag, int wfrag_ready,
                          void* const* outs, int out_dtype, int out_layout, sh_stream_t stream) {
    int rc = check_call(n_steps, steps, rows0, c0, B, x && weights && outs && wfrag, "sh_stack_forward_bf16");
    if (rc != SH_OK) return rc;
    rc = prep_wfrags(n_steps, steps, weights, wfrag, 0, false, wfrag_ready != 0, "sh_stack_forward_bf16", stream);
    if (rc != SH_OK) return rc;
    const void* cur = x;
    int cd = x_dtype;
    Lay cl = lay(x_layout, rows0, B, c0);
    int c = c0;
    for (int i = 0; i < n_steps; ++i) {
        const sh_stack_step& s = steps[i];
        const bool is_last = i == n_steps - 1;
        const int co = s.kind == 0 ? s.cout : c;
        const int od = is_last ? out_dtype : SH_DTYPE_BF16;
        const Lay ol = lay(is_last ? out_layout : 0, out_rows(s), B, co);
        SH_REQUIRE(outs[i], SH_ERR_INVALID_ARG, "sh_stack_forward_bf16: no output buffer for step %d", i);
        if (s.kind == 0) {
            rc = sh_spiral_conv_fwd_bf16(cur, cd, cl.sv, cl.sb, s.table, wfrag[i], biases ? biases[s.param] : nullptr, outs[i], od, ol.sv,
                                         ol.sb, B, s.R, s.S, s.cin, s.cout, s.act, s.zero_row, stream);
        } else {
            SH_REQUIRE(cd == SH_DTYPE_BF16 && od == SH_DTYPE_BF16, SH_ERR_UNSUPPORTED,
                       "sh_stack_forward_bf16: re-sampling step %d needs bf16 on both sides", i);
            if (s.extend) {
                SH_REQUIRE(i > 0 && !is_last && outs[i] == outs[i - 1] && cl.sb == c, SH_ERR_INVALID_ARG,
                           "sh_stack_forward_bf16: step %d appends to its input, which must be the vertex-major output buffer of step %d", i, i - 1);
                rc = sh_spmm_bf16(s.m.rowptr, s.m.col, s.m.val, cur, cl.sv, cl.sb, static_cast<char*>(outs[i]) + (long)s.m_cols * cl.sv * 2, cl.sv,
                                  cl.sb, nullptr, 0, 0, 0, -1, B, s.m_rows, c, stream);
            } else {
                rc = sh_spmm_bf16(s.m.rowptr, s.m.col, s.m.val, cur, cl.sv, cl.sb, outs[i], ol.sv, ol.sb, nullptr, 0, 0, 0, -1, B, s.m_rows, c,
                                  stream);
            }
        }
        if (rc != SH_OK) return rc;
        cur = outs[i]; cd = od; cl = ol; c = co;
    }
    return SH_OK;
}

int sh_stack_backward_bf16(int n_steps, const sh_stack_step* steps, const void* x, int x_dtype, int x_layout, int rows0, int c0, int B,
                           const void* const* acts, const void* g, int out_dtype, int out_layout, const float* const* weights,
                           void* const* gin, int gx_dtype, void* dpre_last, void* const* wfrag_t, int wfrag_ready,
                           void* const* workspace, const size_t* workspace_bytes, float* const* dW, float* const* dbias, int need_x_grad,
                           sh_stream_t stream) {
    int rc = check_call(n_steps, steps, rows0, c0, B, x && acts && g && weights && gin && dW, "sh_stack_backward_bf16");
    if (rc != SH_OK) return rc;
    const int last = n_steps - 1;
    int cin_of[64];
    fill_cin_of(n_steps, steps, c0, cin_of);
    // backward-data operands of all conv steps: one conversion launch
    rc = prep_wfrags(n_steps, steps, weights, wfrag_t, 1, !need_x_grad, wfrag_ready != 0, "sh_stack_backward_bf16", stream);
    if (rc != SH_OK) return rc;
    const void* cur; Lay cl; int cd;
    {
        const sh_stack_step& s = steps[last];
        if (s.kind == 0) {
            SH_REQUIRE(dpre_last, SH_ERR_INVALID_ARG, "sh_stack_backward_bf16: no dpre_last buffer");
            const Lay ol = lay(out_layout, s.R, B, s.cout), dl = lay(0, 0, B, s.cout);
            if (out_dtype == SH_DTYPE_F32)
                rc = sh_act_backward(static_cast<const float*>(g), ol.sv, ol.sb, static_cast<const float*>(acts[last]), ol.sv, ol.sb,
                                     static_cast<float*>(dpre_last), dl.sv, dl.sb, B, s.R, s.cout, s.act, s.zero_row, stream);
            else
                rc = sh_act_backward_bf16(g, ol.sv, ol.sb, acts[last], ol.sv, ol.sb, dpre_last, dl.sv, dl.sb, B, s.R, s.cout, s.act, s.zero_row,
                                          stream);
            if (rc != SH_OK) return rc;
            cur = dpre_last; cl = dl; cd = out_dtype;
        } else {
            SH_REQUIRE(out_dtype == SH_DTYPE_BF16, SH_ERR_UNSUPPORTED, "sh_stack_backward_bf16: a re-sampling last step needs a bf16 gradient");
            cur = g; cl = lay(out_layout, s.m_rows, B, cin_of[last]); cd = out_dtype;
        }
    }
    ReduceJobs jobs;
    for (int i = last; i >= 0; --i) {
        const sh_stack_step& s = steps[i];
        const bool want_in = i > 0 || need_x_grad;
        const void* inp = i == 0 ? x : acts[i - 1];
        const int ind = i == 0 ? x_dtype : SH_DTYPE_BF16;
        const Lay il = i == 0 ? lay(x_layout, rows0, B, c0) : lay(0, 0, B, cin_of[i]);
        void* gi = want_in ? gin[i] : nullptr;
        const int gd = i == 0 ? gx_dtype : SH_DTYPE_BF16;
        SH_REQUIRE(!want_in || gi, SH_ERR_INVALID_ARG, "sh_stack_backward_bf16: no gradient buffer for the input of step %d", i);
        const Lay gl = i == 0 ? lay(x_layout, rows0, B, c0) : lay(0, 0, B, cin_of[i]);
        const void* yprev = nullptr; Lay yl{0, 0}; int act_prev = 0, zero_prev = -1;
        if (i > 0 && steps[i - 1].kind == 0) {
            yprev = acts[i - 1]; yl = lay(0, 0, B, steps[i - 1].cout); act_prev = steps[i - 1].act; zero_prev = steps[i - 1].zero_row;
        }
        if (s.kind == 0) {
            SH_REQUIRE(workspace && workspace[i], SH_ERR_INVALID_ARG, "sh_stack_backward_bf16: no workspace for step %d", i);
            const bool wgrad = dW[s.param] != nullptr;                 // NULL: frozen layer, no weight gradient (see sh_stack_backward)
            SH_REQUIRE(wgrad || !dbias || !dbias[s.param], SH_ERR_INVALID_ARG,
                       "sh_stack_backward_bf16: parameter %d has a dbias buffer but no dW buffer", s.param);
            // role-swapped weight gradient of a 16 -> 3 channel layer (see sh_stack_backward)
            const bool thin = wgrad && want_in && s.table_t && cd == SH_DTYPE_F32 && ind == SH_DTYPE_BF16 && s.R == s.n_in && il.sb == s.cin &&
                              il.sv == (long)B * s.cin && cl.sb == s.cout && cl.sv == (long)B * s.cout &&
                              sh_spiral_conv_bwd_wgt_thin_ok(B, s.n_in, s.S, s.cin, s.cout, SH_DTYPE_BF16);
            if (wgrad && !thin) {
                rc = sh_spiral_conv_bwd_wgt_bf16(cur, cd, cl.sv, cl.sb, inp, ind, il.sv, il.sb, s.table, workspace[i], workspace_bytes[i], B,
                                                 s.R, s.S, s.cin, s.cout, stream);
                if (rc != SH_OK) return rc;
            }
            if (wgrad) jobs.add(workspace[i], dW[s.param], dbias ? dbias[s.param] : nullptr, B, s, 0);
            if (want_in) {
                SH_REQUIRE(s.table_t, SH_ERR_INVALID_ARG, "sh_stack_backward_bf16: step %d has no transposed table", i);
                // backward-data over ragged source lists (round 6): every source a real row of dpre - neither the pre-sum launches nor
                // the empty slots of the dense transposed table (SH_BF16_RAGGED=0: the dense form)
                static const int rag_on = sh_env_int("SH_BF16_RAGGED", 1, 0, 1);
                const bool rag = rag_on && !thin && cd == SH_DTYPE_BF16 && gd == SH_DTYPE_BF16 && s.rag_rows && s.rag_pos &&
                                 sh_spiral_conv_bf16_rag_ok(B, s.S, s.cout, s.cin, s.rag_L);
                char* mut = static_cast<char*>(const_cast<void*>(cur));      // extra rows behind the R real ones of this step's buffer
                const long rb = cl.sv * esz_of(cd);
                for (int lev = 0; lev < 2; ++lev) {
                    const int n = lev == 0 ? s.n1 : s.n2;
                    if (!n || rag) continue;
                    const sh_csr_ref& m = lev == 0 ? s.sum1 : s.sum2;
                    void* dst = mut + (long)(s.R + (lev == 0 ? 0 : s.n1)) * rb;
                    if (cd == SH_DTYPE_F32)
                        rc = sh_spmm(m.rowptr, m.col, m.val, static_cast<const float*>(cur), cl.sv, cl.sb, static_cast<float*>(dst), cl.sv, cl.sb,
                                     nullptr, 0, 0, 0, -1, B, n, s.cout, stream);
                    else
                        rc = sh_spmm_bf16(m.rowptr, m.col, m.val, cur, cl.sv, cl.sb, dst, cl.sv, cl.sb, nullptr, 0, 0, 0, -1, B, n, s.cout, stream);
                    if (rc != SH_OK) return rc;
                }
                const bool thin_dx = thin && gd == SH_DTYPE_BF16 && gl.sb == s.cin && gl.sv == (long)B * s.cin && (!yprev || yprev == inp);
                if (thin) {
                    rc = sh_spiral_conv_bwd_wgt_thin(static_cast<const float*>(cur), cl.sv, cl.sb, inp, SH_DTYPE_BF16, il.sv, il.sb, s.table_t,
                                                     workspace[i], workspace_bytes[i], weights[s.param], thin_dx ? gi : nullptr, gl.sv, gl.sb,
                                                     nullptr, yprev ? act_prev : SH_ACT_IDENTITY, zero_prev, B, s.R, s.n_in, s.S, s.cin, s.cout,
                                                     SH_DTYPE_BF16, stream);
                    if (rc != SH_OK) return rc;
                }
                if (rag)
                    rc = sh_spiral_conv_bwd_data_bf16_rag(cur, cl.sv, cl.sb, s.rag_rows, s.rag_pos, s.rag_L, wfrag_t[i], gi, gl.sv, gl.sb, yprev, yl.sv,
                                                          yl.sb, act_prev, zero_prev, B, s.n_in, s.S, s.cin, s.cout, stream);
                else if (!thin_dx)
                    rc = sh_spiral_conv_bwd_data_bf16(cur, cd, cl.sv, cl.sb, s.table_t, wfrag_t[i], gi, gd, gl.sv, gl.sb, yprev, yl.sv, yl.sb,
                                                      act_prev, zero_prev, B, s.n_in, s.S, s.cin, s.cout, stream);
                if (rc != SH_OK) return rc;
            }
        } else if (want_in) {
            SH_REQUIRE(s.mt.rowptr && s.mt.col && s.mt.val, SH_ERR_INVALID_ARG, "sh_stack_backward_bf16: step %d has no transposed matrix", i);
            SH_REQUIRE(cd == SH_DTYPE_BF16 && gd == SH_DTYPE_BF16, SH_ERR_UNSUPPORTED,
                       "sh_stack_backward_bf16: re-sampling step %d needs bf16 on both sides", i);
            rc = sh_spmm_bf16(s.mt.rowptr, s.mt.col, s.mt.val, cur, cl.sv, cl.sb, gi, gl.sv, gl.sb, yprev, yl.sv, yl.sb, act_prev, zero_prev, B,
                              s.m_cols, cin_of[i], stream);
            if (rc != SH_OK) return rc;
        }
        if (want_in) { cur = gi; cl = gl; cd = gd; }
    }
    return jobs.flush(reduce_bf16, stream);
}

}  // extern "C"
