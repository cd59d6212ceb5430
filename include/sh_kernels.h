/*
 * sh_kernels.h - C ABI of libsh_kernels.so: the MI355X (gfx950) kernels behind the
 * spiral-convolution mesh-autoencoder training path of SemanticHuman.
 *
 * The reference (pure Python/PyTorch) has no FFI layer; its boundary for this path is the
 * nn.Module surface of models.py.  Each entry point below names the reference lines whose
 * ATen dispatches it replaces.  A maintainer binds them with ctypes;
 * semantichuman_amd/_lib.py is exactly that binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch caching allocator); tables are
 *     int32, tensors fp32; nothing is allocated, freed or retained by the library
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it
 *     (no synchronisation, no hipMalloc: safe under hipGraph capture)
 *   - activations are addressed with explicit element strides so one kernel serves both
 *       batch-major  [B][rows][C]  (the reference layout):  sv = C,     sb = rows*C
 *       vertex-major [rows][B][C]  (the fast internal layout): sv = B*C, sb = C
 *     element (row r, batch b, channel c) lives at  base + r*sv + b*sb + c
 *   - return value: 0 on success, negative sh_status on failure (never throws);
 *     sh_last_error() gives a thread-local message
 */
#ifndef SH_KERNELS_H
#define SH_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sh_stream_t;

#if defined(__GNUC__)
#define SH_API __attribute__((visibility("default")))
#else
#define SH_API
#endif

enum sh_status {
    SH_OK = 0,
    SH_ERR_INVALID_ARG = -1,   /* null pointer, negative size, misaligned stride */
    SH_ERR_UNSUPPORTED = -2,   /* shape outside what the kernels were built for */
    SH_ERR_WORKSPACE = -3,     /* workspace too small */
    SH_ERR_LAUNCH = -4         /* hipLaunchKernel reported an error */
};

/* activation ids: the strings reference models.py:19-32 accepts */
enum sh_act {
    SH_ACT_IDENTITY = 0,
    SH_ACT_RELU = 1,
    SH_ACT_ELU = 2,         /* alpha = 1 */
    SH_ACT_LEAKY_RELU = 3,  /* slope 0.02 (models.py:24) */
    SH_ACT_SIGMOID = 4,
    SH_ACT_TANH = 5
};

SH_API int sh_version(void);
SH_API const char* sh_last_error(void);
/* 16 hex digits: SHA-256 over the kernel sources this library was compiled from (csrc/Makefile BUILD_ID).  bench.py quotes
 * a committed PMC profile only for the build it was taken on. */
SH_API const char* sh_build_id(void);

/* Arithmetic form of the fp32 path's matrix products (SpiralConv forward / backward-data / weight gradient).  The
 * reference computes them with fp32 FMAs (models.py:45, aten::addmm).
 *   SH_MMA_EXACT    v_mfma_f32_16x16x4_f32: an exact fp32 FMA chain.
 *   SH_MMA_SPLIT3   every fp32 operand split EXACTLY into three bf16 terms (8+8+8 significand bits), the six leading
 *                   partial products on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; dropped terms < 2^-24 |w||x|,
 *                   i.e. fp32-level error (the parity tolerances in tests/ are the same for all forms); the split is done
 *                   by every consumer on what it gathered.
 *   SH_MMA_PLANES3  the same arithmetic with the split done ONCE, by the producer of a tensor, into three bf16 planes that
 *                   the consumers gather (the ..._p3 entry points at the end of this header; sh_stack_forward /
 *                   sh_stack_backward run them wherever the plane buffers they are given allow, and the SPLIT3 kernels
 *                   elsewhere).  On the per-layer fp32 entry points it selects the SPLIT3 kernels.
 * `mma_mode` is an ARGUMENT of every entry point whose kernel choice depends on it: there is no process-wide setting (a
 * forward pass and the backward pass of another node may run concurrently on different threads in different forms). */
enum sh_mma_mode { SH_MMA_EXACT = 0, SH_MMA_SPLIT3 = 1, SH_MMA_PLANES3 = 2 };

/* Optional per-kernel timing with HIP events attached to the kernel dispatch itself (begin / end of
 * the kernel's execution, what rocprofv3 --kernel-trace reports; minor helper kernels are bracketed
 * by event records on the stream instead).  Used by bench.py for the roofline figures; off by
 * default, must be off while a hipGraph is being captured.  sh_profile_get synchronises on the events. */
/* Diagnostic: shader clock currently granted.  n_workgroups single-wave workgroups each time `iters` dependent fp32
 * MFMAs with the shader-cycle counter and the 100 MHz counter: out[2*i] = shader cycles, out[2*i+1] = 100 MHz ticks
 * (device memory, 2*n_workgroups entries).  tools/clock_probe.py launches it between training steps. */
SH_API int sh_clock_probe(unsigned long long* out, int n_workgroups, int iters, sh_stream_t stream);
SH_API int sh_profile_enable(int on);                 /* on=1 start recording (clears), on=0 stop */
SH_API int sh_profile_count(void);
SH_API int sh_profile_get(int i, char* name, int name_len, float* ms);

/* ---------------------------------------------------------------------------------------------
 * SpiralConv forward.  Replaces models.py:40-51 (aten::index gather, aten::addmm, activation,
 * dummy-row mask) with one fused kernel; the gathered [B*(N+1), S*Cin] matrix is never
 * materialised.
 *   y[r,b,:] = act( sum_s x[table[r,s], b, :] . W[:, s*Cin:(s+1)*Cin]^T + bias )      r < R
 *   y[zero_row,b,:] = 0   (zero_row < 0: no masking)
 * table: int32 [R][S], values in [0, n_in) - the caller has already mapped the reference's -1
 * to the dummy row (torch negative-index wrap, models.py:42).  R may be smaller than n_in: a
 * row-select down-sampling D (models.py:127) is fused by passing table = spirals[sel].
 * weight: [Cout][S*Cin] row-major = nn.Linear.weight (models.py:17); bias may be NULL.
 */
SH_API int sh_spiral_conv_fwd(const float* x, int64_t x_sv, int64_t x_sb,
                       const int32_t* table, const float* weight, const float* bias,
                       float* y, int64_t y_sv, int64_t y_sb,
                       int B, int R, int S, int Cin, int Cout, int act, int zero_row, int mma_mode,
                       sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SpiralConv backward w.r.t. the input.  Replaces autograd's aten::mm (dG = dY.W) +
 * aten::_index_put_impl_(accumulate=True) scatter-add by a GATHER over the
 * transposed table - no atomics, fixed summation order, bitwise reproducible.  It is the same
 * fused gather+MFMA kernel as the forward pass:
 *   dx[u,b,:] = sum_s dpre[table_t[u,s], b, :] . W[:, s*Cin:(s+1)*Cin]            u < n_in
 * table_t: int32 [n_in][S]; table_t[u,s] = the output row r with table[r,s] == u.  Where no such r
 * exists it must point at a row of dpre that is zero (the masked dummy row); where several exist
 * (irregular vertices, the dummy row) the caller first sums those rows of dpre into an extra row
 * (sh_spmm with unit values) and points table_t at it - semantichuman_amd/stack.py does both.
 * weight_t: [Cin][S*Cout], weight_t[ci][s*Cout+co] = weight[co][s*Cin+ci]  (sh_weight_transpose).
 * Optional epilogue (yprev != NULL): dx is multiplied by act_prev'(yprev) evaluated from the
 * OUTPUT yprev of the layer that produced x, and row zero_row is forced to 0, so dx is directly
 * that layer's pre-activation gradient (aten::elu_backward + mask backward).
 */
SH_API int sh_spiral_conv_bwd_data(const float* dpre, int64_t dp_sv, int64_t dp_sb,
                            const int32_t* table_t, const float* weight_t,
                            float* dx, int64_t dx_sv, int64_t dx_sb,
                            const float* yprev, int64_t yp_sv, int64_t yp_sb, int act_prev, int zero_row,
                            int B, int n_in, int S, int Cin, int Cout, int mma_mode,
                            sh_stream_t stream);
/* The same with one more piece of knowledge: row `dpre_zero_row` of dpre is all zero and is the row the "no source" entries
 * of table_t point at (>= 0; -1 = unknown: identical to sh_spiral_conv_bwd_data).  With a batch slice of 16 and gathered
 * channel counts that are multiples of 16 the kernels then skip the matrix products of (vertex, spiral position) pairs
 * without a source - exact zeros: the result is bitwise the same; 51-59 % of the entries on down-sampling levels. */
SH_API int sh_spiral_conv_bwd_data_z(const float* dpre, int64_t dp_sv, int64_t dp_sb, int dpre_zero_row, const int32_t* table_t,
                                     const float* weight_t, float* dx, int64_t dx_sv, int64_t dx_sb, const float* yprev,
                                     int64_t yp_sv, int64_t yp_sb, int act_prev, int zero_row, int B, int n_in, int S, int Cin,
                                     int Cout, int mma_mode, sh_stream_t stream);

/* weight [Cout][S*Cin] -> weight_t [Cin][S*Cout] (see above). */
SH_API int sh_weight_transpose(const float* weight, float* weight_t, int S, int Cin, int Cout, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SpiralConv backward w.r.t. weight and bias.  Replaces aten::mm dW = dY^T.G; the
 * gathered matrix G is re-gathered on the fly.  Two-stage, deterministic: per-block partial
 * slabs in `workspace`, then a fixed-order reduction.
 *   dW[co, s*Cin+ci] = sum_{r,b} dpre[r,b,co] * x[table[r,s], b, ci];   dbias[co] = sum_{r,b} dpre[r,b,co]
 * dbias may be NULL.  Results OVERWRITE dW/dbias.
 */
SH_API size_t sh_spiral_conv_bwd_wgt_workspace(int B, int R, int S, int Cin, int Cout);
SH_API int sh_spiral_conv_bwd_wgt(const float* dpre, int64_t dp_sv, int64_t dp_sb,
                           const float* x, int64_t x_sv, int64_t x_sb, const int32_t* table,
                           float* dW, float* dbias, void* workspace, size_t workspace_bytes,
                           int B, int R, int S, int Cin, int Cout, int mma_mode,
                           sh_stream_t stream);

/* The same launch with a rider: the LAST pre-sum level of the layer's backward-data pass (sh_stack_step.sum1 / sum2: rows
 * R .. of the dpre buffer = sums of rows that several (vertex, position) pairs of the transposed table share) -
 *     sum_out[r][b][:] = sum_e sum_val[e] * dpre[sum_col[e]][b][:]      r < sum_rows, strides of dpre, sh_spmm's arithmetic
 * - computed by extra workgroups of the weight-gradient launch (both only read the first R rows of dpre) instead of a launch of
 * its own, when a second wave of the kernel fits on a SIMD; otherwise the entry point issues sh_spmm itself, first.
 * sum_out_planes != NULL: the three-plane image of those rows (sh_spmm_p3's y_planes) is written with them.
 * sum_rows == 0: exactly sh_spiral_conv_bwd_wgt. */
SH_API int sh_spiral_conv_bwd_wgt_presum(const float* dpre, int64_t dp_sv, int64_t dp_sb, const float* x, int64_t x_sv, int64_t x_sb,
                                         const int32_t* table, float* dW, float* dbias, void* workspace, size_t workspace_bytes,
                                         const int32_t* sum_rowptr, const int32_t* sum_col, const float* sum_val, float* sum_out,
                                         void* sum_out_planes, int sum_rows, int B, int R, int S, int Cin, int Cout, int mma_mode,
                                         sh_stream_t stream);

/* Batched forms for a whole stack of layers (one launch instead of one per layer; host arrays of
 * n_layers entries, passed by value into the kernel arguments -> graph-capturable):
 *  - sh_spiral_conv_bwd_wgt called with dW == NULL only writes its partial slabs into `workspace`;
 *    sh_spiral_conv_bwd_wgt_reduce_multi then reduces the slabs of up to 16 layers (same B,R,S,Cin,Cout
 *    as the producing calls; dbias[i] may be NULL);
 *  - sh_weight_transpose_multi transposes up to 32 weights. */
SH_API int sh_spiral_conv_bwd_wgt_reduce_multi(int n_layers, const void* const* workspaces, float* const* dW,
                                        float* const* dbias, const int* B, const int* R, const int* S,
                                        const int* Cin, const int* Cout, sh_stream_t stream);
SH_API int sh_weight_transpose_multi(int n_layers, const float* const* weight, float* const* weight_t,
                              const int* S, const int* Cin, const int* Cout, sh_stream_t stream);

/* dpre = dy * act'(y) with row zero_row forced to 0 (aten::elu_backward + mask, models.py:46-51). */
SH_API int sh_act_backward(const float* dy, int64_t dy_sv, int64_t dy_sb,
                    const float* y, int64_t y_sv, int64_t y_sb,
                    float* dpre, int64_t dp_sv, int64_t dp_sb,
                    int B, int R, int C, int act, int zero_row, sh_stream_t stream);
/* The same launch with the weight transposes of a stack's backward pass (sh_weight_transpose_multi's arguments) as extra
 * workgroups: both are a few microseconds of work, a launch boundary costs ~3 us whatever follows it.  n_layers == 0:
 * exactly sh_act_backward. */
SH_API int sh_act_backward_tr(const float* dy, int64_t dy_sv, int64_t dy_sb, const float* y, int64_t y_sv, int64_t y_sb,
                       float* dpre, int64_t dp_sv, int64_t dp_sb, int B, int R, int C, int act, int zero_row, int n_layers,
                       const float* const* weight, float* const* weight_t, const int* S, const int* Cin, const int* Cout,
                       sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Sparse mesh re-sampling.  Replaces the dense aten::bmm of models.py:127 (D) and :148 (U), and
 * with the transposed CSR their backward:
 *   y[r,b,:] = sum_{e in [rowptr[r], rowptr[r+1])} val[e] * x[col[e], b, :]
 * Optional epilogue as in sh_spiral_conv_bwd_data (yprev != NULL).
 */
SH_API int sh_spmm(const int32_t* rowptr, const int32_t* col, const float* val,
            const float* x, int64_t x_sv, int64_t x_sb,
            float* y, int64_t y_sv, int64_t y_sb,
            const float* yprev, int64_t yp_sv, int64_t yp_sb, int act_prev, int zero_row,
            int B, int rows, int C, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Whole-stack execution.  The reference runs encode / decode as Python loops over layers
 * (models.py:119-128 conv + D per level, :146-153 U + conv per level) and leaves the backward chain to
 * autograd; issued call by call from Python that is ~25 us of host time per launch (measured), i.e. the
 * host, not the GPU, paces an eagerly launched step.  These two entry points issue the launches of a
 * whole stack - forward, or the hand-scheduled backward chain - from one call.  They only sequence the
 * entry points above (same kernels, same results, same launch order as calling them one by one), never
 * allocate and never synchronise: every buffer is the caller's.
 *
 * A step is a SpiralConv (kind 0; a row-select D is already folded into `table`) or a sparse
 * re-sampling (kind 1).  Layouts: 0 = vertex-major [rows][B][C] (all internal tensors), 1 = batch-major
 * [B][rows][C] (allowed for the stack input and the stack output only).
 */
typedef struct sh_csr_ref { const int32_t* rowptr; const int32_t* col; const float* val; } sh_csr_ref;
typedef struct sh_stack_step {
    int kind;                         /* 0 conv, 1 spmm */
    int param;                        /* conv: index into the weights / biases / dW / dbias arrays */
    /* conv */
    const int32_t* table;             /* [R][S] */
    const int32_t* table_t;           /* [n_in][S] transposed table (see sh_spiral_conv_bwd_data) */
    int R, S, n_in, cin, cout, act, zero_row;
    int n1, n2;                       /* extra rows of the pre-activation gradient buffer: list pre-sums, levels 1 and 2 */
    sh_csr_ref sum1, sum2;            /* their unit-valued CSR (n1 / n2 rows) */
    /* spmm */
    sh_csr_ref m, mt;                 /* y = M x and its transpose */
    int m_rows, m_cols;
    /* extend != 0: the step follows a conv whose output buffer has room for m_rows more rows behind its m_cols real ones;
     * M (m_rows x m_cols) holds only the NON-identity rows of the up-sampling and the forward pass appends M x there: the
     * next step reads Z = [x ; M x] (m_cols + m_rows rows) through a table composed with the row map, outs[i] must equal
     * outs[i-1], and mt is the transpose of [I ; M] (m_cols x (m_cols + m_rows)), so the backward pass is the plain one. */
    int extend;
    /* conv, optional (round 6; NULL / 0 = none): the step's backward-data sources as RAGGED lists instead of table_t + pre-summed
     * rows - rag_rows [n_in][rag_L]: for input row u its sources (rows of the pre-activation gradient, all < R), rag_pos [n_in][rag_L]:
     * the spiral position whose weight multiplies each, -1 behind a row's last source (rag_rows then holds any valid row).  A step
     * that has them and whose backward-data pass runs on planes with a resident weight (sh_spiral_conv_p3_rag_ok) takes
     * sh_spiral_conv_bwd_data_p3_rag and needs neither its pre-sum launches nor the extra rows filled. */
    const int32_t* rag_rows;
    const int32_t* rag_pos;
    int rag_L;
    /* conv, optional (round 6; NULL / 0 = none): GROUPED lists - output rows whose source lists overlap share one list of the union
     * (mesh_ops.group_lists; sh_spiral_conv_p3_grp).  fg_*: the forward pass (groups of rows of the step's output, sources = rows of
     * its input, built from `table`); bg_*: the backward-data pass (groups of rows of the step's input, sources = rows of the
     * pre-activation gradient, built from the ragged lists).  x_rows [n][L] rows of the gathered tensor; x_pos [n][L] one byte per
     * member: the spiral position that member reads the row at, 0xFF = it does not (0xFFFFFFFF behind the group's last entry);
     * x_out [n][4] the members' output rows (-1: none; at most sh_spiral_conv_p3_grp_members() of them).  A step that has them and
     * whose pass runs on planes with a resident weight (sh_spiral_conv_p3_grp_ok) takes the grouped kernel: every row of a group's
     * union is gathered once (SH_P3_GROUPED=0: the one-row lists / the table). */
    const int32_t* fg_rows; const uint32_t* fg_pos; const int32_t* fg_out; int fg_n, fg_L;
    const int32_t* bg_rows; const uint32_t* bg_pos; const int32_t* bg_out; int bg_n, bg_L;
} sh_stack_step;

/* The kernel forms of an fp32 stack (sh_stack_forward / sh_stack_backward), decided in one place for both passes: from the steps, c0,
 * B, x_layout, mma_mode, keep_fp32 (the forward pass's; the backward pass's acts_fp32), need_x_grad and the switches SH_P3_N16_MAXB,
 * SH_P3_WGRAD, SH_P3_DROP_FP32, SH_P3_RAGGED, SH_P3_GROUPED.
 * sh_stack_plan_f32 writes per step an OR of SH_FORM_* flags (backward flags as a layer with a weight gradient runs them).  Both
 * sequencers compute this plan and require the per-step buffers it names (SH_ERR_INVALID_ARG when one is NULL); a caller sizes its
 * buffers from it. */
enum sh_stack_form {
    SH_FORM_FWD_P3 = 1,                /* conv: forward on the plane image of its input (planes[i - 1], wfrag3[i]) */
    SH_FORM_FWD_GRP = 2,               /* ... over grouped lists */
    SH_FORM_FWD_IMG = 4,               /* the step writes the plane image of its output (planes[i]) */
    SH_FORM_FWD_IMG_ONLY = 8,          /* ... and leaves its fp32 rows unwritten */
    SH_FORM_BWD_GIMG = 16,             /* the pre-activation gradient gets an image (gin_planes[i + 1] / dpre_last_planes, wfrag3_t[i]) */
    SH_FORM_BWD_THIN = 32,             /* role-swapped weight gradient, which computes the input gradient too */
    SH_FORM_BWD_P3 = 64,               /* backward-data on planes */
    SH_FORM_BWD_RAG = 128,             /* ... over ragged source lists */
    SH_FORM_BWD_GRP = 256,             /* ... over grouped lists */
    SH_FORM_BWD_RIDE = 512,            /* the last pre-sum level rides in the weight-gradient launch */
    SH_FORM_BWD_PRESUM_IMG = 1024,     /* the pre-summed gradient rows get an image */
    SH_FORM_BWD_P3W = 2048,            /* weight gradient from the two images (in_planes[i]) */
    SH_FORM_BWD_YIMG = 4096,           /* plane backward-data takes the activation derivative from the input's image (in_planes[i]) */
    SH_FORM_BWD_IN_IMG_ONLY = 8192,    /* keep_fp32 == 2: the step's input may be its image alone */
    SH_FORM_BWD_GRAD_IMG_ONLY = 16384  /* keep_fp32 == 2: its pre-activation gradient is handed over as the image alone */
};
SH_API int sh_stack_plan_f32(int n_steps, const sh_stack_step* steps, int c0, int B, int x_layout, int mma_mode, int keep_fp32,
                             int need_x_grad, int* forms);

/* outs[i]: output of step i, vertex-major, except outs[n_steps-1] which has layout out_layout.
 * x: [rows0] rows of c0 channels in layout x_layout. */
/* Three-plane form (mma_mode == SH_MMA_PLANES3 and both arrays given; NULL arrays: no plane form): planes[i] = buffer for the plane
 * image of outs[i] (sh_p3_bytes of the buffer's rows - a step that appends shares its predecessor's buffer AND image), required where
 * the plan says SH_FORM_FWD_IMG; wfrag3[i] = three-plane weight fragments of conv step i, forward operand
 * (sh_conv_wfrag3_prep_multi, transpose 0), already converted from the CURRENT weights, required where it says SH_FORM_FWD_P3.
 * keep_fp32: 1 = every step writes its fp32 output (a backward pass reads them); 0 = forward only: rows that the next plane
 * conv gathers through their image alone are written as the image alone (SH_FORM_FWD_IMG_ONLY; the last step's output is always
 * fp32); 2 (round 6) = training on the images: the same rows, where the BACKWARD pass of the conv that gathers them leaves their fp32
 * form unread as well (SH_FORM_BWD_IN_IMG_ONLY); the caller of 2 owes sh_stack_backward the plane buffers and acts_fp32 == 2. */
SH_API int sh_stack_forward(int n_steps, const sh_stack_step* steps, const float* x, int x_layout, int rows0, int c0, int B,
                            const float* const* weights, const float* const* biases, float* const* outs, int out_layout,
                            int mma_mode, void* const* planes, const void* const* wfrag3, int keep_fp32, sh_stream_t stream);

/* acts[i]: what sh_stack_forward wrote to outs[i].  g: gradient w.r.t. the stack output (out_layout).
 * gin[i]: gradient w.r.t. the INPUT of step i - for i >= 1 vertex-major with (n1 + n2 of step i-1, if that is a
 * conv) extra rows behind the real ones, for i == 0 layout x_layout, NULL when need_x_grad == 0; buffers of
 * non-adjacent steps may alias (gin[i] is dead once gin[i-1] has been produced).  dpre_last: as gin[] for the
 * output of the last step when that is a conv ([R + n1 + n2][B][cout]), else unused.  Per conv step i:
 * weight_t[i] ([cin][S*cout], needed when i > 0 or need_x_grad), workspace[i] / workspace_bytes[i]
 * (>= sh_spiral_conv_bwd_wgt_workspace); per parameter index: dW[p], dbias[p] (may be NULL).
 * Three-plane form (SH_MMA_PLANES3 with gin_planes and wfrag3_t; NULL arrays: no plane form): where the plan says SH_FORM_BWD_GIMG,
 * gin_planes[i + 1] / dpre_last_planes = buffer for the plane image of the step's pre-activation gradient (all rows, the pre-summed
 * ones included) and wfrag3_t[i] = fragments of its backward-data operand (transpose 1); weight_t[i] may then be NULL unless the
 * step is SH_FORM_BWD_THIN.  in_planes (round 6; NULL: the forward images were not kept): in_planes[i] = the plane image of the
 * INPUT of conv step i - what sh_stack_forward wrote to planes[i - 1], kept alive by the caller - required where the plan says
 * SH_FORM_BWD_P3W or SH_FORM_BWD_YIMG; the plan names only images the forward pass wrote.  SH_FORM_BWD_P3W computes the step's
 * WEIGHT gradient from the two images (sh_spiral_conv_bwd_wgt_p3_presum) when its workspace has at least
 * sh_spiral_conv_bwd_wgt_p3_workspace() bytes, else from the fp32 tensors (sh_spiral_conv_bwd_wgt_presum).  acts_fp32: the
 * keep_fp32 sh_stack_forward ran with (1 or 2).  With 2 (plane form and in_planes required) a step whose input was left as its
 * image alone must run on the images: SH_ERR_INVALID_ARG when it cannot (never a read of unwritten rows); and the gradient rows
 * this pass hands from step to step are written as their image alone where the plan says SH_FORM_BWD_GRAD_IMG_ONLY.
 * dW[p] == NULL (the dW array itself is required) means: do not compute the weight gradient of the conv step(s) of parameter p
 * (a frozen layer; dbias[p] must then be NULL too).  Such a step launches no weight-gradient kernel and has no job in the slab
 * reduction; what used to ride in that launch runs on its own: the last pre-sum level as the standalone sh_spmm_p3 launch, the
 * role-swapped 16 -> 3 layer's input gradient as the ordinary backward-data kernel.  Weight transposes / fragments are still
 * made (backward-data reads them).  A forward pass whose backward pass will skip a step must run with keep_fp32 == 1 (the
 * skipped step reads fp32 rows), and this call then gets acts_fp32 == 1. */
SH_API int sh_stack_backward(int n_steps, const sh_stack_step* steps, const float* x, int x_layout, int rows0, int c0, int B,
                             const float* const* acts, const float* g, int out_layout, const float* const* weights,
                             float* const* gin, float* dpre_last, float* const* weight_t, void* const* workspace,
                             const size_t* workspace_bytes, float* const* dW, float* const* dbias, int need_x_grad,
                             int mma_mode, void* const* gin_planes, void* dpre_last_planes, const void* const* wfrag3_t,
                             const void* const* in_planes, int acts_fp32, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Dense layers with one tiny and one huge dimension: the latent nn.Linear pair fc_latent_enc /
 * fc_latent_dec (models.py:85-86, applied at :130 and :144) and their autograd.  Contiguous
 * row-major tensors; weight is nn.Linear.weight [N][K].  All three stream the weight-shaped matrix
 * once (HBM-bound); a reduction that is too long for one workgroup is split over workgroups into
 * partial slabs in `workspace` (>= sh_linear_workspace bytes) and summed in a fixed order.
 *   fwd       y[M,N]  = x[M,K] . weight^T + bias        (bias may be NULL)
 *   bwd_data  dx[M,K] = dy[M,N] . weight
 *   bwd_wgt   dW[N,K] = dy^T . x ;  dbias[N] = column sums of dy (dbias may be NULL)
 * mma_mode (enum sh_mma_mode, round 5): SH_MMA_EXACT = fp32 MFMA; SH_MMA_SPLIT3 / SH_MMA_PLANES3 = both fp32 operands split
 * exactly into three bf16 terms inside the kernel, six partial products on the bf16 MFMA, fp32 accumulation (batch <= 64 and the
 * streaming kernels' shapes; other shapes run the fp32 MFMA kernels whatever the mode).  Nothing is written in bf16.
 */
SH_API size_t sh_linear_workspace(int M, int N, int K);
SH_API int sh_linear_fwd(const float* x, const float* weight, const float* bias, float* y, int M, int N, int K,
                  void* workspace, size_t workspace_bytes, int mma_mode, sh_stream_t stream);
SH_API int sh_linear_bwd_data(const float* dy, const float* weight, float* dx, int M, int N, int K,
                       void* workspace, size_t workspace_bytes, int mma_mode, sh_stream_t stream);
SH_API int sh_linear_bwd_wgt(const float* dy, const float* x, float* dW, float* dbias, int M, int N, int K,
                      void* workspace, size_t workspace_bytes, int mma_mode, sh_stream_t stream);
/* Weight gradient of a latent FC with torch.optim.Adam's update applied to it in the same kernel (round 5): every 64 x 64 tile of
 * dW = dy^T . x is, instead of being stored, used as the gradient `g` of sh_adam_step's update of the same tile of `weight`,
 * `exp_avg` and `exp_avg_sq` (in place; coefficients from the DEVICE scalars `step` = updates applied so far and `lr`, so the
 * launch is replayable in a hipGraph).  Bit-identical to sh_linear_bwd_wgt followed by sh_adam_step on that tensor (one shared
 * update function), without writing and re-reading the gradient: 24 instead of 32 bytes of HBM traffic per weight.  `step` is
 * NOT advanced here (every workgroup reads it): the caller advances it once the launch is queued (sh_adam_bump, or a numel == 0 entry of sh_adam_step).  dbias as in
 * sh_linear_bwd_wgt (the bias keeps its ordinary gradient).  Served shapes: sh_linear_bwd_wgt_adam_ok (M <= 64, N and K
 * multiples of 64); others return SH_ERR_UNSUPPORTED and nothing is launched.
 * Replaces, for one parameter, the pair reference `loss.backward()` (models.py:130 / :144 autograd of nn.Linear) +
 * `optimizer.step()` (train_funcs.py:391-392, 509-510).  Only valid when nothing else consumes that gradient between backward
 * and step (no all-reduce, clipping or accumulation over several backward passes).
 * dy / x carry an element type (enum sh_dtype, declared below): bf16 operands (the bf16 path's layer, sh_linear_bwd_wgt_bf16) are
 * widened to fp32 in the kernel and multiplied on the fp32 MFMA - exact products of bf16 values, fp32 accumulation; `weight_bf16`,
 * if not NULL, is the bf16 working copy of the weight and is rewritten with the update (as sh_adam_step_bf16 does). */
SH_API int sh_linear_bwd_wgt_adam_ok(int M, int N, int K);
SH_API int sh_linear_bwd_wgt_adam(const void* dy, int dy_dtype, const void* x, int x_dtype, float* weight, void* weight_bf16, float* exp_avg,
                           float* exp_avg_sq, const float* step, const float* lr, double beta1, double beta2, double eps,
                           double weight_decay, float* dbias, int M, int N, int K, int mma_mode, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Grouped (ragged) dense layers: the 3 x 17 per-part nn.Linear layers of SpiralAutoencoder_multiz_partkps
 * (models.py:200-204, applied one at a time at :236, :252, :269) in ONE launch per direction.  All groups read their
 * inputs from, and write their outputs to, column ranges of two row-major matrices:
 *   fwd       y[m][y_off[g] + n]  = sum_k x[m][x_off[g] + k] * W_g[n][k] + bias_g[n]            n < N[g], k < K[g]
 *   bwd_data  dx[m][x_off[g] + k] = sum_n dy[m][y_off[g] + n] * W_g[n][k]
 *   bwd_wgt   dW_g[n][k] = sum_m dy[m][y_off[g] + n] * x[m][x_off[g] + k];   dbias_g[n] = sum_m dy[m][y_off[g] + n]
 * x / dx have row stride x_rs, y / dy row stride y_rs (elements).  w, bias, dW, dbias, x_off, y_off, N, K are HOST
 * arrays of G entries (device pointers / element offsets / sizes); bias, dbias and their entries may be NULL.
 * W_g is [N[g]][K[g]] row-major (nn.Linear.weight).  Deterministic; results overwrite their outputs.
 */
SH_API int sh_grouped_linear_fwd(int G, const float* x, int64_t x_rs, const int64_t* x_off, const float* const* w,
                          const float* const* bias, float* y, int64_t y_rs, const int64_t* y_off, int M,
                          const int* N, const int* K, sh_stream_t stream);
SH_API int sh_grouped_linear_bwd_data(int G, const float* dy, int64_t y_rs, const int64_t* y_off, const float* const* w,
                               float* dx, int64_t x_rs, const int64_t* x_off, int M, const int* N, const int* K,
                               sh_stream_t stream);
SH_API int sh_grouped_linear_bwd_wgt(int G, const float* dy, int64_t y_rs, const int64_t* y_off, const float* x,
                              int64_t x_rs, const int64_t* x_off, float* const* dW, float* const* dbias, int M,
                              const int* N, const int* K, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Losses / metric.  All reductions are two-stage with a fixed order (no atomics).
 * workspace: at least sh_reduce_workspace() bytes.
 */
SH_API size_t sh_reduce_workspace(void);

/* loss[0] = mean |a - b| over n elements           (F.l1_loss, train_funcs.py:501) */
SH_API int sh_l1_loss_fwd(const float* a, const float* b, int64_t n, float* loss, void* workspace, sh_stream_t stream);
/* grad_b[i] = sign(b[i]-a[i]) * gscale[0] / n      (gscale: device scalar = upstream gradient) */
SH_API int sh_l1_loss_bwd(const float* a, const float* b, int64_t n, const float* gscale, float* grad_b, sh_stream_t stream);

/* out[0] = mean_{b<B, v<N} | scale * (a[b,v,:3] - b[b,v,:3]) |_2  for contiguous [B][N1][3] tensors,
 * rows v >= N (the dummy row) excluded                           (test_funcs.py:41-49) */
SH_API int sh_vertex_l2(const float* a, const float* b, int B, int N1, int N, float scale, float* out,
                 void* workspace, sh_stream_t stream);

/* Edge-length-ratio regulariser (train_funcs.py:12-39, 503-508), batched on device:
 *   loss[0] = mean_{b,f} sum_{e in 3 edges} | |e_rec| / (|e_gt| + 1e-5) - 1 |
 * x_hat, x: contiguous [B][N1][3]; faces int32 [F][3].
 * bwd: corner lists (vptr [N1+1], vcorner [3F], entries f*3+k) give an atomic-free gradient
 *   grad[b,v,:] = gscale[0]/(B*F) * sum_{corners of v} d score / d x_hat[b,v,:]
 * STATED DEVIATION from the reference on one edge case (here and in sh_recon_loss_bwd): a RECONSTRUCTED edge of length exactly 0.
 * The reference differentiates torch.sqrt(torch.sum(d ** 2)) (train_funcs.py:36-38) at d = 0: autograd multiplies the sqrt's
 * infinite derivative by 2 d = 0 and every gradient of that batch entry downstream becomes NaN - the optimizer step then turns
 * the whole model into NaN.  These kernels return the term's subgradient 0 for such an edge (`if (len > 0)`), so a collapsed
 * face contributes its loss value (|0 / t - 1| = 1) and no gradient, and training continues.  Everywhere else (len > 0) the
 * gradient is the reference's.  tests/test_gpu_parity.py::test_zero_length_reconstructed_edge pins both behaviours. */
SH_API int sh_edge_ratio_loss_fwd(const float* x_hat, const float* x, const int32_t* faces, int B, int N1, int F,
                           float* loss, void* workspace, sh_stream_t stream);
SH_API int sh_edge_ratio_loss_bwd(const float* x_hat, const float* x, const int32_t* faces,
                           const int32_t* vptr, const int32_t* vcorner, int B, int N1, int F,
                           const float* gscale, float* grad, sh_stream_t stream);

/* The reconstruction loss of the plain training loop in one piece (train_funcs.py:501-508):
 *   total[0] = parts[0] + edge_w * parts[1],  parts[0] = mean |x - x_hat| (all N1 rows),  parts[1] = the edge-ratio term above;
 * bwd writes grad = gscale[0] * d total / d x_hat.  Three launches instead of eleven; same arithmetic as the separate
 * kernels.  workspace: sh_recon_loss_workspace() bytes.
 * bwd takes the vertex -> neighbour lists instead of the corner lists: vptr [N1+1] counts the corners of every vertex (as
 * above), vnbr int32 [2 * 3F] holds, corner by corner in that order, the two other vertices of the corner's face
 * (faces[f][(k+1)%3], faces[f][(k+2)%3]) - the same sum in the same order without the corner -> face indirection. */
SH_API size_t sh_recon_loss_workspace(void);
SH_API int sh_recon_loss_fwd(const float* x_hat, const float* x, const int32_t* faces, int B, int N1, int F, float edge_w,
                      float* total, float* parts, void* workspace, sh_stream_t stream);
SH_API int sh_recon_loss_bwd(const float* x_hat, const float* x, const int32_t* vptr, const int32_t* vnbr, int B, int N1, int F,
                      float edge_w, const float* gscale, float* grad, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Part-wise pairwise-distance loss of the semantic training loop (train_funcs.py:243-284 and
 * :353-389; utils_distance.calc_euclidean_dist_matrix :366-376; utils_SH.angle_skl :442-478).
 * For every part p, batch entry b and ordered vertex pair (i,j), i != j, of the part:
 *   De = |g_i-g_j| * scale[b,p];  De_r = |r_i-r_j|;  w from the angle between (g_i-g_j) and bone[b,p]
 *   (w_mode 0 all_one, 1 angle/90, 2 sin(angle), 3 angle/90 thresholded at w_threshold; flags[p]&1
 *   forces w = 1); pairs with w*De == 0 are dropped;
 *   term = relat ? |w*De_r/De - w| : |w*De_r - w*De|;   loss = sum_p w_part[p] * mean_{kept pairs} term.
 * x_rec, x_gt: contiguous [B][N1][3]; bone [B][P][3]; scale [B][P] or NULL (= 1); parts as CSR
 * (part_ptr [P+1], part_vert), disjoint; tile_ptr [P+1] = cumulative ceil(n_p / sh_part_pairdist_tile_rows());
 * T = tile_ptr[P]; max_part = largest n_p.  workspace >= B*T*2 floats.  part_sum / part_cnt [P] are
 * outputs of fwd; bwd takes part_cnt, a device scalar gscale, and OVERWRITES grad [B][N1][3]
 * (gradient w.r.t. x_rec; vertices outside every part get 0).  Deterministic (no atomics).
 */
SH_API int sh_part_pairdist_tile_rows(void);
SH_API int sh_part_pairdist_loss_fwd(const float* x_rec, const float* x_gt, const float* bone, const float* scale,
                              const int32_t* part_ptr, const int32_t* part_vert, const int32_t* tile_ptr,
                              const int32_t* flags, const float* w_part, int B, int N1, int P, int T, int max_part,
                              int w_mode, float w_threshold, int relat, float* loss, float* part_sum, float* part_cnt,
                              void* workspace, size_t workspace_bytes, sh_stream_t stream);
SH_API int sh_part_pairdist_loss_bwd(const float* x_rec, const float* x_gt, const float* bone, const float* scale,
                              const int32_t* part_ptr, const int32_t* part_vert, const int32_t* tile_ptr,
                              const int32_t* flags, const float* w_part, int B, int N1, int P, int T, int max_part,
                              int w_mode, float w_threshold, int relat, const float* part_cnt, const float* gscale,
                              float* grad, sh_stream_t stream);
/* The forward pass that also leaves the backward pass's row sums: grad_raw [B][N1][3] (rows of part vertices written, the
 * rest untouched) = pairdist's gradient without the factor 2 gscale w_p / count_p, which only exists once the counts are
 * complete; sh_part_pairdist_loss_bwd_scale applies it (grad: cleared, then the part vertices' rows written;
 * n_part_verts = part_ptr[P]) - the same bits as sh_part_pairdist_loss_bwd, without its second sweep over the pairs.
 * grad_raw == NULL: exactly sh_part_pairdist_loss_fwd. */
SH_API int sh_part_pairdist_loss_fwd_grad(const float* x_rec, const float* x_gt, const float* bone, const float* scale,
                                   const int32_t* part_ptr, const int32_t* part_vert, const int32_t* tile_ptr, const int32_t* flags,
                                   const float* w_part, int B, int N1, int P, int T, int max_part, int w_mode, float w_threshold,
                                   int relat, float* loss, float* part_sum, float* part_cnt, float* grad_raw, void* workspace,
                                   size_t workspace_bytes, sh_stream_t stream);
SH_API int sh_part_pairdist_loss_bwd_scale(const float* grad_raw, const int32_t* part_ptr, const int32_t* part_vert,
                                   const float* w_part, const float* part_cnt, const float* gscale, int B, int N1, int P,
                                   int n_part_verts, float* grad, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Body measurements (utils_SH.py:86-98 cal_length, :144-161 measure_body_quick; numpy twins
 * obj2npy.py:61-79), batched over meshes.
 * Girth of ring p = length of the CLOSED polyline through its n_p points
 *   q_i = v[ring_a[i]] * (1 - ring_f[i]) + v[ring_b[i]] * ring_f[i],   i in [ring_ptr[p], ring_ptr[p+1])
 * (utils_SH.py:155-158: closing segment q_0-q_last plus the n_p-1 consecutive ones).
 * v: [B] meshes of [*][3] floats, batch stride v_sb floats; girth [B][P].
 * Bone length p = | k[bones[3p]] - k[bones[3p+1]] |, or, when bones[3p+2] >= 0,
 *   | k[bones[3p]] - (k[bones[3p+1]] + k[bones[3p+2]]) / 2 |   (utils_SH.py:94-97);
 * kps contiguous [B][K][3]; bones int32 [P][3]; length [B][P].
 */
SH_API int sh_measure_girth(const float* v, int64_t v_sb, const int32_t* ring_ptr, const int32_t* ring_a,
                     const int32_t* ring_b, const float* ring_f, int B, int P, float* girth, sh_stream_t stream);
SH_API int sh_bone_length(const float* kps, const int32_t* bones, int B, int K, int P, float* length, sh_stream_t stream);
/* Their gradients (fp32, deterministic: gather form over transposed lists the host builds once - measure.py GirthRings / Bones;
 * every term of an output row is summed in list order, no atomics; plain stores of every element of the output).
 *  - sh_measure_girth_bwd: g_girth [B][P] -> g_v contiguous [B][rows][3] (OVERWRITTEN).  pt_ring [n_points] = ring of each ring
 *    point; vt_ptr [n_vt + 1] / vt_pt / vt_w: CSR over vertex rows of (ring point k, weight) with weight 1 - ring_f[k] for
 *    ring_a[k] and ring_f[k] for ring_b[k], entries of a row ordered by k (a before b); n_vt <= rows, rows >= n_vt get 0.
 *    Segment k joins point k and point (k+1) mod n as in sh_measure_girth (n == 1: length 0; n == 2: the two points twice); a
 *    zero-length segment has subgradient 0.  v / v_sb as for sh_measure_girth.
 *  - sh_bone_length_bwd: g_len [B][P] -> g_kps contiguous [B][K][3] (OVERWRITTEN).  jt_ptr [n_jt + 1] / jt_bone / jt_w: CSR over
 *    joints of (bone, signed weight): +1 for the head, -1 for a 2-joint bone's tail, -1/2 for each tail joint of a 3-joint bone;
 *    entries ordered by bone.  Joints >= n_jt get 0; a zero-length bone has subgradient 0.
 *  - sh_joint_regress_bwd: g_kps contiguous [B][K][3] -> g_x contiguous [B][rows][3] = J^T g_kps for rows < N (J dense [K][N],
 *    joints summed in order), 0 for N <= row < rows (the dummy row). */
SH_API int sh_measure_girth_bwd(const float* v, int64_t v_sb, const int32_t* ring_ptr, const int32_t* ring_a, const int32_t* ring_b,
                                const float* ring_f, const int32_t* pt_ring, const int32_t* vt_ptr, const int32_t* vt_pt,
                                const float* vt_w, int n_vt, const float* g_girth, int B, int P, int rows, float* g_v, sh_stream_t stream);
SH_API int sh_bone_length_bwd(const float* kps, const int32_t* bones, const int32_t* jt_ptr, const int32_t* jt_bone, const float* jt_w,
                              int n_jt, const float* g_len, int B, int K, int P, float* g_kps, sh_stream_t stream);
SH_API int sh_joint_regress_bwd(const float* g_kps, const float* J, int B, int N, int K, int rows, float* g_x, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Nearest points and Chamfer loss: the objective of fitting the model to an unregistered point cloud (no reference
 * counterpart).  All of it fp32, deterministic (no float atomics), plain stores of every output element.
 *
 * sh_nearest_points.  q: [B] bodies of [*][3] query points, batch stride q_sb floats, nq rows searched; t: the same for the
 * targets (t_sb, nt).  q_count / t_count: int32 [B] live rows per body, or NULL (= nq / nt); a count is clamped to [0, rows].
 * t_mask: uint8 [nt] (mask_sb == 0: one mask for all bodies) or [B] masks with stride mask_sb >= nt, 0 = target not allowed;
 * NULL = all allowed.  For body b and query j < q_count[b], over the allowed targets i < t_count[b]:
 *     dx = qx - tx;  dy = qy - ty;  dz = qz - tz          (each rounded to fp32)
 *     d2(i) = fma(dz, dz, fma(dy, dy, dx * dx))           (fp32, two fused multiply-adds on the rounded product dx * dx)
 *     d2[b][j] = min_i d2(i);   idx[b][j] = the lowest i that attains it
 * i.e. the minimum of (d2, i) in lexicographic order - never the expanded |q|^2 + |t|^2 - 2 q.t form, and no other form is used
 * to discard candidates.  A body with no allowed target gets idx = -1, d2 = +inf (so does a query all of whose distances
 * overflow to +inf); queries j >= q_count[b] get idx = -1, d2 = 0.  idx / d2: contiguous [B][nq].
 * The targets may be split into `chunks` contiguous ranges searched by different workgroups and merged by a second kernel
 * (chunks = 0: chosen from B, nq, nt so that the chip is filled - sh_nearest_points_chunks tells; a request is rounded to whole
 * LDS tiles).  The lexicographic minimum is associative and commutative: every split returns the same bits.  A split into more
 * than one chunk needs sh_nearest_points_workspace(B, nq, nt, chunks) bytes.
 * B == 0 or nq == 0: SH_OK, nothing launched.  Negative B, nq, nt or chunks: SH_ERR_INVALID_ARG.
 *
 * sh_chamfer_fwd.  d2_sm [B][M] (scan -> model: queries = scan points, targets = model vertices), s_count [B] or NULL = m_b;
 * d2_ms [B][rows] (model -> scan; read only when w_ms > 0, may be NULL otherwise); v_mask over the first n <= rows model
 * vertices as t_mask above, active = unmasked.  With n_act = active vertices among the first n and tau2 = squared truncation
 * distance (+inf: none):
 *     L[b] = (1/m_b) sum_{j < m_b} min(d2_sm[b][j], tau2)  +  w_ms (1/n_act) sum_{i < n active} min(d2_ms[b][i], tau2)
 * (m_b == 0: L[b] = 0; n_act == 0: no second term).  Sums in fp64 in a fixed order (thread t: terms t, t + 256, ...; then the
 * 256 thread sums in a fixed tree).  counts [B][2] int32 receives (m_b, n_act) for the backward pass.
 *
 * sh_chamfer_bwd.  Gradient w.r.t. the model points x [B][*][3] (stride x_sb, `rows` rows) through the recorded indices; the
 * scan s [B][*][3] (stride s_sb, M rows) takes none.  For i < n active, with k = idx_ms[b][i]:
 *     acc   = sum over j < m_b with idx_sm[b][j] == i and d2_sm[b][j] < tau2, in ascending j, of (x_i - s_j)      (fp32)
 *     g_x[b][i] = gL[b] * ( (2/m_b) acc + [w_ms > 0, d2_ms[b][i] < tau2] (w_ms 2/n_act) (x_i - s_k) )
 * and 0 for every other row (rows >= n, masked vertices, vertices nothing points at, m_b == 0).  g_x: contiguous [B][rows][3],
 * every element stored.  idx_ms / d2_ms may both be NULL when w_ms == 0.  Gather form: a workgroup owns 256 rows, sweeps the
 * indices of the body once and sums its rows' terms in ascending j.
 */
SH_API int sh_nearest_points_chunks(int B, int nq, int nt);
SH_API size_t sh_nearest_points_workspace(int B, int nq, int nt, int chunks);
SH_API int sh_nearest_points(const float* q, int64_t q_sb, int nq, const int32_t* q_count, const float* t, int64_t t_sb, int nt,
                             const int32_t* t_count, const uint8_t* t_mask, int64_t mask_sb, int B, int chunks, int32_t* idx,
                             float* d2, void* workspace, size_t workspace_bytes, sh_stream_t stream);
SH_API int sh_chamfer_fwd(const float* d2_sm, int M, const int32_t* s_count, const float* d2_ms, int rows, int n,
                          const uint8_t* v_mask, int64_t mask_sb, float tau2, float w_ms, int B, float* loss, int32_t* counts,
                          sh_stream_t stream);
SH_API int sh_chamfer_bwd(const float* x, int64_t x_sb, int rows, int n, const float* s, int64_t s_sb, int M, const int32_t* s_count,
                          const int32_t* idx_sm, const float* d2_sm, const int32_t* idx_ms, const float* d2_ms, const uint8_t* v_mask,
                          int64_t mask_sb, const int32_t* counts, float tau2, float w_ms, const float* gL, int B, float* g_x,
                          sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Nearest surface points: the scan -> model term measured to the model's SURFACE instead of to its vertices (no reference
 * counterpart).  fp32, deterministic, plain stores of every output element.
 *
 * sh_nearest_surface.  q: [B] bodies of [*][3] scan points, batch stride q_sb floats, nq rows searched, q_count int32 [B] live
 * rows per body or NULL (= nq).  x: [B] bodies of model points, batch stride x_sb, the first n rows are vertices.  faces: int32
 * [nF][3], ONE table for the whole batch, indices into the first n rows.  v_mask as t_mask of sh_nearest_points, over n rows.  A
 * triangle is a target only if its three indices lie in [0, n) and all three vertices are active; the others are skipped.
 * For scan point s and target triangle f with corners a = x[f0], b = x[f1], c = x[f2], everything in fp32, every operation
 * rounded on its own except the fused multiply-adds written out (no other contraction):
 *     ab = b - a;  ac = c - a;  ap = s - a                               (component-wise: the differences from a come first)
 *     dot(u, v) = fma(u.z, v.z, fma(u.y, v.y, u.x * v.x))
 *     e11 = dot(ab, ab);  e12 = dot(ab, ac);  e22 = dot(ac, ac);  d1 = dot(ab, ap);  d2 = dot(ac, ap)
 *     d3 = d1 - e11;  d4 = d2 - e12;  d5 = d1 - e12;  d6 = d2 - e22      (Ericson's ab.bp, ac.bp, ab.cp, ac.cp, in a's frame)
 *     vc = d1 * d4 - d3 * d2;  vb = d5 * d2 - d1 * d6;  va = d3 * d6 - d5 * d4
 * The region test of Ericson, Real-Time Collision Detection 5.1.5; the FIRST rule that applies gives the weights (v, w) of b, c:
 *     1. d1 <= 0 and d2 <= 0                               (0, 0)                                vertex a
 *     2. d3 >= 0 and d4 <= d3                              (1, 0)                                vertex b
 *     3. vc <= 0 and d1 >= 0 and d3 <= 0                   (d1 / (d1 - d3), 0)                   edge ab
 *     4. d6 >= 0 and d5 <= d6                              (0, 1)                                vertex c
 *     5. vb <= 0 and d2 >= 0 and d6 <= 0                   (0, d2 / (d2 - d6))                   edge ca
 *     6. va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0         w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w      edge bc
 *     7. otherwise, with sum = (va + vb) + vc              (vb * (1 / sum), vc * (1 / sum))      interior
 * An edge rule (3, 5, 6) applies only if its quotient's denominator is > 0, and 1 / sum is replaced by 0 when sum is not > 0.
 * That is the rule for a degenerate triangle (two or three equal corners, or collinear): an edge of length 0 is passed over,
 * the other vertex and edge rules cover the triangle, and where rounding lets a point reach rule 7 it falls to vertex a.  Then v = min(max(v, 0), 1), w = min(max(w, 0), 1 - v): every result is a valid convex
 * combination, l1 = v, l2 = w, l0 = fl(fl(1 - v) - w) >= 0, and every d2 is finite.
 *     r = ap - fma(w, ac, v * ab)   (component-wise);    d2(f) = fma(r.z, r.z, fma(r.y, r.y, r.x * r.x))
 * The answer for the point is the minimum of (d2, f) in lexicographic order: face [B][nq] int32, d2 [B][nq], uv [B][nq][2] =
 * (l1, l2) of that face.  No target triangle: face -1, d2 +inf, uv 0; points j >= q_count[b]: face -1, d2 0, uv 0.
 *
 * How it is computed.  Three launches.  (1) Per body and triangle, the record (a, ab, ac, e11, e12, e22) and a bounding sphere:
 * centre m = a + (ab + ac) / 3, radius SH_SURFACE_MARGIN * sqrt(max |corner - m|^2).  (2) The sweep: scan points in registers
 * (a wave owns 256 consecutive ones), spheres streamed through LDS.  With cull != 0 a triangle is skipped for a point when
 *     |s - m|^2 > (rb + radius)^2,      rb = SH_SURFACE_MARGIN * sqrt(min(bound[b][j], best d2 found so far))
 * all in the difference form above; the region test runs, for the lanes that cannot skip, when any lane of the wave cannot.
 * bound [B][nq] (or NULL = none) is an upper bound of the answer supplied by the caller - the squared distance to the nearest
 * vertex, which sh_nearest_points gives.  Why a skip never changes the result: the computed foot point is a convex combination
 * of the rounded ab, ac, so sqrt(d2(f)) >= dist(s, triangle) (1 - 5 u) - 12 u radius with u = 2^-24, dist(s, triangle) >=
 * |s - m| - radius, and the computed sphere test carries another 4 u: about 30 u in all against the margin's 2^-10 = 16384 u.
 * A skipped triangle is therefore strictly farther than SH_SURFACE_MARGIN times the bound in force.  (3) Per point: the minimum
 * over the chunks; if it exceeds SH_SURFACE_MARGIN * bound[b][j] (the bound was no upper bound after all: a vertex mask can
 * leave the nearest vertex without a target triangle; the factor admits a foot point on the nearest vertex itself, whose
 * distance differs from the vertex search's by rounding) the point is swept again without any bound; then the weights of the
 * chosen face.  cull == 0 runs every (point, triangle) pair through the region test and ignores bound: the
 * yardstick, same bits.  The triangles may be split into `chunks` ranges (0: chosen to fill the chip;
 * sh_nearest_surface_chunks tells) - every split gives the same bits.  workspace: sh_nearest_surface_workspace(B, nq, nF,
 * chunks) bytes, 16-byte aligned, always needed; nothing allocates.  stats: NULL, or two zeroed uint64 that receive [0] the
 * number of (point, triangle) region tests the sweep ran and [1] the number of points swept again in step (3) - a diagnostic
 * for benchmarks, served by a separate instantiation of the sweep (integer atomics, one per wave; the instantiation a NULL
 * selects has no counter and no atomic; results are the same).  B == 0 or nq == 0: SH_OK, nothing launched.
 *
 * sh_chamfer_surface_bwd.  The gradient of sh_chamfer_fwd fed with the d2 above, w.r.t. x, the weights taken as constants
 * (at the minimiser the derivative through them vanishes or is blocked by the active constraint).  For row i < n active:
 *     acc = sum over j < m_b with face[b][j] >= 0, d2[b][j] < tau2 and corner k of that face == i, in ascending j and corner
 *           order 0, 1, 2 within a j, of  fl(l_k * e),   e = fma(w, ac, v * ab) - ap  (= q_j - s_j, from x and uv as above),
 *           (l_0, l_1, l_2) = (fl(fl(1 - v) - w), v, w);          acc = fl(acc + term), no contraction
 *     g_x[b][i] = gL[b] * ( (2/m_b) acc + [w_ms > 0, d2_ms[b][i] < tau2] (w_ms 2/n_act) (x_i - s_k) ),   k = idx_ms[b][i]
 * and 0 for every other row; the model -> scan term is the vertex term of sh_chamfer_bwd, unchanged.  Gather form, a workgroup
 * owns 256 rows; no atomics of any kind.  counts as sh_chamfer_fwd wrote them.
 */
#define SH_SURFACE_MARGIN (1.0f + 0x1p-10f)
SH_API int sh_nearest_surface_chunks(int B, int nq, int nF);
SH_API size_t sh_nearest_surface_workspace(int B, int nq, int nF, int chunks);
SH_API int sh_nearest_surface(const float* q, int64_t q_sb, int nq, const int32_t* q_count, const float* x, int64_t x_sb, int n,
                              const int32_t* faces, int nF, const uint8_t* v_mask, int64_t mask_sb, const float* bound, int B,
                              int chunks, int cull, int32_t* face, float* d2, float* uv, uint64_t* stats, void* workspace,
                              size_t workspace_bytes, sh_stream_t stream);
SH_API int sh_chamfer_surface_bwd(const float* x, int64_t x_sb, int rows, int n, const float* s, int64_t s_sb, int M,
                                  const int32_t* s_count, const int32_t* faces, int nF, const int32_t* face, const float* d2,
                                  const float* uv, const int32_t* idx_ms, const float* d2_ms, const uint8_t* v_mask, int64_t mask_sb,
                                  const int32_t* counts, float tau2, float w_ms, const float* gL, int B, float* g_x,
                                  sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Vertex normals: the two normal fields a scan match is gated by, and the gated search (no reference counterpart).  fp32,
 * deterministic (no atomics of any kind), plain stores of every output element.
 *
 * sh_vertex_normals.  x: [B] bodies of model points, batch stride x_sb floats, the first n rows are vertices.  faces int32
 * [nF][3], ONE table for the batch, indices in [0, n).  The vertex-to-face incidence is CSR: vf_ptr int32 [n + 1], vf_idx int32
 * [3 nF]; vf_idx[vf_ptr[v] .. vf_ptr[v + 1]) are the faces that name vertex v, in ascending face order.  For vertex v, one
 * thread walks its faces in that order; for face f with corners a = x[f0], b = x[f1], c = x[f2] in the face's own corner order,
 * everything in fp32, every operation rounded on its own except the fused multiply-adds written out (no other contraction):
 *     ab = b - a;  ac = c - a                                             (component-wise)
 *     cx = fma(ab.y, ac.z, -(ab.z * ac.y));  cy = fma(ab.z, ac.x, -(ab.x * ac.z));  cz = fma(ab.x, ac.y, -(ab.y * ac.x))
 *     s = fl(s + c)                          (component-wise, starting from 0: the cross products carry the area weights)
 *     len2 = fma(s.z, s.z, fma(s.y, s.y, s.x * s.x))
 *     normal[b][v] = s / sqrtf(len2)  (three divisions) when 0 < len2 < +inf, otherwise (0, 0, 0)
 * The zero vector means "unknown": a vertex in no face, a fan of zero-area faces, an overflow.  normals: contiguous [B][n][3],
 * every element stored; no vertex mask takes part (normals belong to the whole mesh).  A table entry outside its range (face
 * >= nF, corner >= n) is passed over.  B == 0 or n == 0: SH_OK, nothing launched.
 *
 * sh_nearest_points_gated.  sh_nearest_points with a gate on the pair: qn [B] bodies of [*][3] query normals (stride qn_sb, row
 * j belongs to query j), tn the same for the targets (tn_sb), cos_min the gate.  Target i is COMPATIBLE with query j iff
 *     fma(qn.z, tn.z, fma(qn.y, tn.y, qn.x * tn.x)) >= cos_min            (fp32; a NaN compares false)
 * A zero normal on either side gives 0: compatible only when cos_min <= 0.  The answer is the minimum of (d2, i) in
 * lexicographic order over the allowed AND compatible targets, d2(i) the expression of sh_nearest_points, unchanged.  A live
 * query with no such target gets idx = -1, d2 = +inf; queries j >= q_count[b] get idx = -1, d2 = 0.  cos_min = -inf opens the
 * gate: the result is sh_nearest_points' bits (for normals free of NaN).  Chunks, workspace (sh_nearest_points_workspace) and
 * the merge are those of sh_nearest_points; every split returns the same bits.  cos_min NaN: SH_ERR_INVALID_ARG.
 */
SH_API int sh_vertex_normals(const float* x, int64_t x_sb, int n, const int32_t* faces, int nF, const int32_t* vf_ptr,
                             const int32_t* vf_idx, int B, float* normals, sh_stream_t stream);
SH_API int sh_nearest_points_gated(const float* q, int64_t q_sb, int nq, const int32_t* q_count, const float* qn, int64_t qn_sb,
                                   const float* t, int64_t t_sb, int nt, const int32_t* t_count, const float* tn, int64_t tn_sb,
                                   const uint8_t* t_mask, int64_t mask_sb, float cos_min, int B, int chunks, int32_t* idx, float* d2,
                                   void* workspace, size_t workspace_bytes, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Nearest surface points under a normal gate: sh_nearest_surface restricted, per (point, triangle) pair, to the triangles
 * whose FACE normal agrees with the scan point's normal (no reference counterpart).  fp32, deterministic, plain stores of every
 * output element.
 *
 * Face normals.  sh_face_normals: x, x_sb, n, faces, nF as sh_nearest_surface takes them; one thread per (body, face).  For face
 * f with corners a = x[f0], b = x[f1], c = x[f2] in the face's own corner order, everything in fp32, every operation rounded on
 * its own except the fused multiply-adds written out (no other contraction):
 *     ab = b - a;  ac = c - a                                             (component-wise)
 *     cx = fma(ab.y, ac.z, -(ab.z * ac.y));  cy = fma(ab.z, ac.x, -(ab.x * ac.z));  cz = fma(ab.x, ac.y, -(ab.y * ac.x))
 *     len2 = fma(cz, cz, fma(cy, cy, cx * cx))
 *     normal[b][f] = (cx, cy, cz) / sqrtf(len2)  (three divisions) when 0 < len2 < +inf, otherwise (0, 0, 0)
 * - the cross product is the one "Vertex normals" sums.  A face with a corner outside [0, n) gets (0, 0, 0); no vertex mask
 * takes part.  normals: contiguous [B][nF][3], every element stored; no LDS, no atomics.  B == 0 or nF == 0: SH_OK, nothing
 * launched.  (The fp64-normalised face normal of the point-to-plane step below is a different quantity and is left as it is.)
 *
 * sh_nearest_surface_gated.  sh_nearest_surface's arguments, plus qn [B] bodies of [*][3] scan normals (stride qn_sb, row j
 * belongs to point j), fn contiguous [B][nF][3] face normals (sh_face_normals of the same x and faces) and cos_min.  Face f is
 * COMPATIBLE with point j iff
 *     fma(qn.z, fn.z, fma(qn.y, fn.y, qn.x * fn.x)) >= cos_min            (fp32; a NaN compares false)
 * A zero normal on either side gives 0: compatible only when cos_min <= 0.  The answer is the minimum of (d2, f) in
 * lexicographic order over the triangles that are targets (sh_nearest_surface's rule) AND compatible; d2(f) and uv are
 * sh_nearest_surface's, unchanged.  A live point with no such triangle gets face -1, d2 +inf, uv 0 (sh_chamfer_fwd counts it as
 * truncated, sh_chamfer_surface_bwd and the alignment moments drop it); points j >= q_count[b]: face -1, d2 0, uv 0.  cos_min =
 * -inf opens the gate: sh_nearest_surface's bits (for normals free of NaN).  cos_min NaN: SH_ERR_INVALID_ARG.
 *
 * How it is computed.  The three launches of sh_nearest_surface in their gated instantiations, and between the first and the
 * second the search that supplies the bound.  (1) also writes every target triangle's sphere centre m on its own, [B][nF][3],
 * with a flag that is 0 for a triangle that is no target (or whose centre overflowed).  (1b) bound == NULL and cull != 0:
 * sh_nearest_points_gated over those centres with fn as the targets' normals and the flags as the mask gives bound[b][j] = the
 * squared distance to the nearest centre of a compatible target, +inf when there is none.  The nearest-vertex distance is no
 * bound here: the nearest vertex may belong to incompatible faces only.  A centre lies on its face (to rounding), so its
 * distance bounds the gated answer from above.  A caller's bound (non-NULL) is used as it is instead; whatever it holds, step
 * (3) keeps the result exact.  (2) The sphere test is sh_nearest_surface's; a triangle that passes it is region-tested by a lane
 * only if it is compatible with that lane's point, so an incompatible pair neither becomes the best nor tightens rb.  (3) The
 * minimum over the chunks; a result above SH_SURFACE_MARGIN * bound[b][j] is swept again over the compatible targets without a
 * bound.  A point WITHOUT a face whose bound is +inf is not swept again: nothing was skipped because of the bound, so "no
 * compatible target" is exact.  cull == 0: every compatible (point, target) pair is region-tested, bound is ignored and (1b) is
 * not run - the yardstick, same bits.  chunks, stats and the alignment of the workspace as sh_nearest_surface;
 * workspace: sh_nearest_surface_gated_workspace(B, nq, nF, chunks) bytes (it holds the centres, the flags, the bound and the
 * bounding search's own workspace as well).  The split is sh_nearest_surface_chunks'.  No atomics outside the stats counters.
 */
SH_API int sh_face_normals(const float* x, int64_t x_sb, int n, const int32_t* faces, int nF, int B, float* normals,
                           sh_stream_t stream);
SH_API size_t sh_nearest_surface_gated_workspace(int B, int nq, int nF, int chunks);
SH_API int sh_nearest_surface_gated(const float* q, int64_t q_sb, int nq, const int32_t* q_count, const float* qn, int64_t qn_sb,
                                    const float* x, int64_t x_sb, int n, const int32_t* faces, int nF, const float* fn,
                                    const uint8_t* v_mask, int64_t mask_sb, float cos_min, const float* bound, int B, int chunks,
                                    int cull, int32_t* face, float* d2, float* uv, uint64_t* stats, void* workspace,
                                    size_t workspace_bytes, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Cloud normals: the normals of a bare point cloud, estimated from the cloud itself - per point the k nearest points of its own
 * body and the direction of least spread among them (no reference counterpart).  Deterministic: no atomics, every sum in a fixed
 * order, plain stores of every output element; the bits depend on neither batch, padding nor launch shape.
 *
 * sh_cloud_normals.  s: [B] bodies of [*][3] points, batch stride s_sb floats, M rows, count int32 [B] live rows per body or NULL
 * (= M), clamped to [0, M]; SH_CLOUD_K_MIN <= k <= SH_CLOUD_K_MAX.
 * Neighbourhood of point j of body b with m_b live points: k_eff = min(k, m_b);
 *     r2[j]  = the k_eff-th smallest value of d2(s_j, s_i) over all live i - d2 the expression of sh_nearest_points with q = s_j,
 *              t = s_i; the point itself is among the i, at distance 0
 *     member = every live i with d2(s_j, s_i) <= r2[j];        cnt[j] = the number of members (>= k_eff)
 * Ties at the k-th distance are all members: the set depends on neither visiting order nor index.
 * Moments.  Per member d = s_i - s_j component-wise in fp32 (the differences d2 forms, up to sign), each component widened to
 * fp64, where products of two of them are exact.  Nine fp64 running sums per point - S1 = sum d (3), S2 = sum d d^T (6: xx xy xz
 * yy yz zz) - each sum = fl(sum + term), members taken in ascending i, plus the count.  No contraction (none would change a bit:
 * the products are exact).
 * Normal, fp64, no contraction:  mean = S1 / cnt;  C_ab = S2_ab / cnt - mean_a mean_b;  C is diagonalised by cyclic Jacobi
 * rotations in the order (0,1) (0,2) (1,2), SH_CLOUD_JACOBI_SWEEPS sweeps, no convergence test (the rotation of sh_align_solve: t
 * = sign(tau) / (|tau| + sqrt(1 + tau^2)), tau = (a_qq - a_pp) / (2 a_pq), the identity when a_pq == 0).  Cyclic Jacobi
 * converges quadratically once the off-diagonal mass is below the eigenvalue gaps; from any symmetric 3 x 3 start four sweeps
 * bring it below 2^-53 of the norm in every case tried (tests/test_cloud_normals_host.py measures it on the test clouds and on
 * random and degenerate matrices), and the count is twice that.  Eigenvalues l0 <= l1 <= l2 are the diagonal, l0 the smallest
 * with the lowest index on a tie; the normal is the eigenvector column of l0, divided by its fp64 length.
 * Unknown - a row of exact zeros, var 0 - when cnt < 3 or !(l1 > SH_CLOUD_RANK_MIN * l2): coincident or collinear
 * neighbourhoods, and any NaN.
 * Sign.  The component of largest magnitude (fp64; the lowest index on a tie) is made positive, then each component is rounded
 * to fp32 once: canonical, UNORIENTED.  With a viewpoint v (view != NULL; for point j it is view[b * view_sb + j * view_ps ..
 * + 3): view_ps == 0 one viewpoint per body, view_ps == 3 one per point) the rounded normal n is negated when
 *     (n_x (v_x - s_x) + n_y (v_y - s_y)) + n_z (v_z - s_z) < 0             (fp64 from the fp32 values, no contraction)
 * exactly 0 (or NaN) keeps the canonical sign.
 * Surface variation: var[j] = max(l0, 0) / ((l0 + l1) + l2) in fp64, rounded to fp32: 0 on a plane, 1/3 at most.
 * Outputs: nrm contiguous [B][M][3]; var, r2 fp32 and cnt int32, each contiguous [B][M] and each optional (NULL: not written).
 * Rows j >= m_b hold zeros in every output.  Without r2 the k-th distances still have to live somewhere between the two
 * launches: workspace, B * M * sizeof(float) bytes; with r2 given the workspace is not used.
 *
 * How it is computed.  Two launches, both in the form of the nearest search: queries in registers, the body's points streamed
 * through LDS tiles, every lane reading the same address.  (1) cloud_kth_kernel keeps per query a sorted list of DISTANCES ONLY
 * in registers, of capacity CAP = 8 / 16 / 32 / 64 (the first at or above k): CAP - k_eff slots are pre-filled with -inf, k_eff
 * with +inf, and a candidate below the last slot is inserted through an unrolled median-of-three chain - the last slot is
 * always the k_eff-th smallest value so far.  The insertion stands under a wave ballot.  1, 2 or 4 queries per thread, chosen
 * from B and M to fill the chip; the k-th smallest of a set depends on none of it.  (2) cloud_normals_kernel sweeps the body
 * once more in ascending i with the compare d2 <= r2[j] on every candidate and the fp64 sums under a wave ballot, never split
 * over target ranges, and finishes each point in its own thread.  No atomics, no scratch memory.
 * Brute force: O(m_b^2) distances per body, meant to run once per scan.  B == 0 or M == 0: SH_OK, nothing launched.  k out of
 * range, a null s or nrm, negative sizes, strides shorter than a body or viewpoint strides that fit neither layout:
 * SH_ERR_INVALID_ARG before the device is touched.
 */
#define SH_CLOUD_K_MIN 3
#define SH_CLOUD_K_MAX 64
#define SH_CLOUD_JACOBI_SWEEPS 8
#define SH_CLOUD_RANK_MIN 1e-12
SH_API int sh_cloud_normals(const float* s, int64_t s_sb, int M, const int32_t* count, int B, int k, const float* view,
                            int64_t view_sb, int64_t view_ps, float* nrm, float* var, float* r2, int32_t* cnt, void* workspace,
                            size_t workspace_bytes, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Vertex visibility: which model vertices a sensor at a known position sees - the vertex mask of a partial (one-view) scan (no
 * reference counterpart).  fp32, deterministic (no atomics of any kind), plain stores of every output element; the bits depend
 * on neither batch, launch shape nor split.
 *
 * sh_vertex_visibility.  x: [B] bodies of model points, batch stride x_sb floats, the first n rows are vertices; rows >= n (the
 * decoder's dummy row) are never read.  faces int32 [nF][3], ONE table for the batch; a face with a corner outside [0, n) is
 * passed over.  view: fp32 [B][3] contiguous, the sensor's position per body in the frame of x.  mask as t_mask of
 * sh_nearest_points, over n rows.  vis: uint8 [B][n] contiguous, 1 = visible.
 * Unknown viewpoint.  A vertex whose mask is 0 is not visible.  A body whose viewpoint row holds a NaN has no viewpoint: all its
 * active vertices are visible, nothing else is looked at (one batch may mix partial and full scans).
 * Occlusion.  For vertex i with o = x_i and d = v_b - o (component-wise, fp32) the vertex is occluded when the open segment
 * o + t d, 0 < t < 1, meets a face that does not name vertex i.  EVERY face of the table occludes, whatever the mask says:
 * masked geometry is still in the way.  Faces that name i are skipped BY INDEX, not by arithmetic (for the origin at corner c,
 * t = e2 . (e2 x e1) is no exact zero in fp32).  The test is Moeller-Trumbore without a division; for the face's corners a, b,
 * c in the face's own order, everything in fp32, every operation rounded on its own except the fused multiply-adds written out
 * (no other contraction - the rule of nn_d2 and of the region test of "Nearest surface points"):
 *     dot(u, v)   = fma(u.z, v.z, fma(u.y, v.y, u.x * v.x))
 *     cross(u, v) = (fma(u.y, v.z, -(u.z * v.y)),  fma(u.z, v.x, -(u.x * v.z)),  fma(u.x, v.y, -(u.y * v.x)))
 *     e1 = b - a;  e2 = c - a;  s = o - a                                  (component-wise)
 *     p = cross(d, e2);  det = dot(e1, p);  u = dot(s, p);  q = cross(s, e1);  w = dot(d, q);  t = dot(e2, q)
 *     sigma = -1 when det < 0, else +1;   |det| = fabs(det)
 *     hit  iff  det != 0  and  sigma u >= 0  and  sigma w >= 0  and  fl(sigma u + sigma w) <= |det|  and  0 < sigma t < |det|
 * (sigma applied by negation, which is exact; a NaN compares false: no hit).  Edges and corners of a face belong to it; the two
 * ends of the segment do not.  Two distinct vertices at (nearly) the same place may hide each other's faces or not: ambiguous
 * by nature, as is a ray along an edge.
 * Facing (tn != NULL).  tn: contiguous [B][n][3] unit vertex normals (sh_vertex_normals of the same x).  The vertex must also
 * face the sensor:   dot(tn_i, d) >= fl(cos_g * sqrtf(dot(d, d)))        (a NaN compares false: not visible)
 * cos_g in [0, 1) is the cosine of the largest angle between normal and line of sight; a zero ("unknown") normal passes only
 * for cos_g == 0, as with the gates.  tn == NULL: no normal is read, cos_g is ignored.
 * visible = active and facing (if asked) and not occluded.
 *
 * How it is computed.  The form of the nearest search: 256 threads, one vertex per thread in registers; faces streamed through
 * double-buffered LDS tiles of 256 - each thread gathers one face's corners from x and stores (a, e1, e2, i0, i1, i2), 48 bytes,
 * and the inner loop reads a face as three 16-byte reads at an address common to all lanes.  Any-hit: a lane is done once it is
 * hit, masked, beyond n or turned away; a wave stops testing when a ballot finds every lane done, and the tile loop ends
 * for the workgroup when all four waves are (the fetch of the next tile, already in flight by then, is dropped).  The face range may be split into `chunks` ranges of whole tiles (0: chosen from B, n, nF to fill the
 * chip, the rule of sh_nearest_points); each chunk then stores its flag into workspace [chunks][B][n] bytes and a second launch
 * ORs them - no atomics, and an OR depends on no order, so every split returns the same bits.  A split into more than one chunk
 * needs sh_vertex_visibility_workspace(B, n, nF, chunks) bytes.  Brute force: O(n nF) tests per body before the early exits.
 * B == 0 or n == 0: SH_OK, nothing launched.  Null x / view / vis, negative sizes, a stride shorter than a body, cos_g outside
 * [0, 1) with tn: SH_ERR_INVALID_ARG before the device is touched.
 */
SH_API size_t sh_vertex_visibility_workspace(int B, int n, int nF, int chunks);
SH_API int sh_vertex_visibility(const float* x, int64_t x_sb, int n, const int32_t* faces, int nF, const float* tn, const float* view,
                                float cos_g, const uint8_t* mask, int64_t mask_sb, int B, int chunks, void* workspace,
                                size_t workspace_bytes, uint8_t* vis, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Vertex visibility from a rig: which model vertices AT LEAST ONE of V sensors sees - the vertex mask of a scan fused from a rig
 * of depth cameras.  Everything of "Vertex visibility" holds: fp32, no atomics, plain stores, bits independent of batch, launch
 * shape and split.
 *
 * sh_vertex_visibility_views.  The arguments of sh_vertex_visibility, with view: fp32 [B][V][3] contiguous, 1 <= V <=
 * SH_VISIBILITY_MAX_VIEWS, and a second output seen: uint32 [B][n] contiguous, or NULL.
 * Bit v of seen[b][i] is set iff vertex i is active and, for view v ALONE, faces the sensor (if tn is given) and is not occluded:
 * the predicate of "Vertex visibility" with d = view[b][v] - o, the same dot / cross forms, the same Moeller-Trumbore
 * expression, incident faces skipped by index - so bit v equals, bit for bit, what sh_vertex_visibility returns when given view v
 * alone.  A view row that holds a NaN is an absent camera: its bit is never set.  vis[b][i] = (seen[b][i] != 0), except for a
 * body ALL of whose view rows hold a NaN: it is a full scan, seen is 0 and every active vertex is visible (the single-view rule;
 * V == 1 reproduces sh_vertex_visibility).
 *
 * How it is computed.  ONE sweep over the faces in the form of the single-view kernel (256 threads, one vertex per thread, the
 * same double-buffered 256-face LDS tiles of 48 bytes).  Per face and vertex s = o - a, q = cross(s, e1) and t = dot(e2, q) do
 * not depend on the view and are formed once; p, det, u and w are formed per view.  A lane carries the 32-bit mask of the views
 * it is still unoccluded from - live and facing, minus hits - and walks its set bits only; the viewpoints sit in LDS (16 bytes
 * per view) and d is formed again from them.  The wave's ballot ("any view open") every four faces and the workgroup's exit per
 * tile work as in the single-view kernel.  `chunks` splits the face range as there; each chunk then stores the views its faces
 * hide into workspace uint32 [chunks][B][n] and a second launch ORs them and takes them off "live and facing", formed again -
 * every split gives the same bits.  sh_vertex_visibility_views_workspace(B, n, nF, V, chunks) bytes are needed for a split into
 * more than one chunk.
 * B == 0 or n == 0: SH_OK, nothing launched.  What sh_vertex_visibility refuses, and V outside [1, SH_VISIBILITY_MAX_VIEWS]:
 * SH_ERR_INVALID_ARG before the device is touched.
 */
#define SH_VISIBILITY_MAX_VIEWS 32
SH_API size_t sh_vertex_visibility_views_workspace(int B, int n, int nF, int V, int chunks);
SH_API int sh_vertex_visibility_views(const float* x, int64_t x_sb, int n, const int32_t* faces, int nF, const float* tn, const float* view,
                                      int V, float cos_g, const uint8_t* mask, int64_t mask_sb, int B, int chunks, void* workspace,
                                      size_t workspace_bytes, uint8_t* vis, uint32_t* seen, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Scan alignment: the similarity that carries a scan into the model's frame, from the matches the search above has recorded
 * (no reference counterpart).  A pose maps scan frame -> model frame, s' = A s + t with A = c R, R a proper rotation, c > 0.
 * Stored fp32: pose contiguous [B][12] (A row-major, then t) and scale [B] (= c).  No atomics; every sum in a fixed order.
 *
 * sh_align_moments.  s [B][*][3] the (aligned) scan, stride s_sb, M rows, s_count [B] or NULL = m_b; x [B][*][3] the model
 * points, stride x_sb, `rows` rows, the first n of them vertices; v_mask, idx_sm / d2_sm [B][M], idx_ms / d2_ms [B][rows], tau2,
 * w_ms as sh_chamfer_bwd takes them (idx_ms / d2_ms may be NULL when w_ms == 0).  The pairs (p = scan side, q = model side) and
 * weights are those of the Chamfer loss:
 *     scan -> model:  (s_j, x[idx_sm[j]])  for j < m_b with 0 <= idx_sm[j] < n and d2_sm[j] < tau2,             weight 1 / m_b
 *     model -> scan:  (s[idx_ms[i]], x_i)  for active i < n with 0 <= idx_ms[i] < m_b and d2_ms[i] < tau2,  weight w_ms / n_act
 * (the second only when w_ms > 0).  Stage 1, this call: one workgroup per range of SH_ALIGN_RANGE consecutive j (then i); thread
 * t takes t, t + 256, ... of its range, fp64 products of the fp32 coordinates, fp64 sums, then a fixed tree over the 256
 * threads.  partials: fp64 [B][sh_align_ranges(M, n, w_ms)][SH_ALIGN_PARTIAL], per range the UNWEIGHTED sums
 *     [0] pairs kept  [1..3] sum p  [4..6] sum q  [7..15] sum q p^T (row-major: q_r p_c at 7 + 3 r + c)  [16] sum |p|^2
 *     [17] sum |q|^2  [18] active vertices of the range (model -> scan ranges only)
 * every element stored (a range beyond m_b holds zeros).  The order depends on M and n only, never on B or the grid.
 *
 * sh_align_moments_surface.  sh_align_moments with the scan -> model partner on the model's SURFACE: idx_sm / d2_sm give way to
 * what sh_nearest_surface recorded - faces int32 [nF][3] (one table for the batch), face [B][M], uv [B][M][2], d2 [B][M] (the
 * surface distance).  A scan -> model pair j < m_b is kept iff 0 <= face[j] < nF, the face's three corner indices lie in [0, n)
 * and d2[j] < tau2 (strict; the vertex mask is not consulted: the search has already refused a triangle with a masked corner).
 * Its pair is (p, q) = (s_j, q_j), weight 1 / m_b, q_j the foot point: with a, b, c the corners x[f0], x[f1], x[f2] in the
 * face's order and (v, w) = uv[j], per coordinate k
 *     ab_k = fl32(b_k - a_k);  ac_k = fl32(c_k - a_k)                                (fp32, the differences of the search)
 *     q_k = (double)a_k + ((double)v * (double)ab_k + (double)w * (double)ac_k)      (fp64, no contraction: two exact products,
 *                                                                                     two rounded additions)
 * The sums, the partials' layout, the ranges, the grid and the order are those of sh_align_moments; so are the model -> scan
 * ranges (vertex x_i to scan point s[idx_ms[i]], as the model -> scan term of the surface Chamfer loss), and sh_align_solve
 * finishes either call's partials.  nF >= 0; nF == 0 keeps no scan -> model pair.  One kernel template serves both calls.
 *
 * sh_align_solve.  Stage 2 and the closed form, one wave per body.  The ranges' sums are added in range order per direction and
 * joined with the weights above into the moments, mom fp64 [B][SH_ALIGN_MOMENTS] (optional output):
 *     [0] W = sum w  [1..3] sum w p  [4..6] sum w q  [7..15] sum w q p^T  [16] sum w |p|^2  [17] sum w |q|^2  [18] pairs kept
 *     [19] 0
 * Then, in fp64: p_bar = sum w p / W, q_bar likewise, H = sum w q p^T / W - q_bar p_bar^T; R = the rotation of Horn's closed form
 * (the eigenvector of the largest eigenvalue of the symmetric 4 x 4 matrix built from H, cyclic Jacobi, SH_ALIGN_JACOBI_SWEEPS
 * sweeps, no convergence test), a proper rotation for every H; c = trace(R^T H) / var_p with var_p = sum w |p|^2 / W - |p_bar|^2
 * for SH_ALIGN_SIMILARITY (c = 1 when var_p <= 0 or the numerator <= 0, and in the other modes); R = I for SH_ALIGN_TRANSLATION;
 * t = q_bar - c R p_bar.  W == 0: the increment is the identity.  inc (optional) fp32 [B][13] receives the increment (c R
 * row-major, t, c).  The pose so far (pose_in [B][12], scale_in [B]) is composed with it, A_new = c R A_old,
 * t_new = c R t_old + t, scale_new = c scale_old, each rounded to fp32 once, into pose_out / scale_out (may alias the inputs;
 * pose_out NULL: only mom is written).  M, n, s_count and w_ms must be those of the sh_align_moments call.
 *
 * sh_transform_points.  dst contiguous [B][M][3]; for j < count[b] (NULL = M), with p = src[b][j] (stride src_sb) and the pose:
 *     dst[b][j][r] = fma(A[r][2], p_z, fma(A[r][1], p_y, fma(A[r][0], p_x, t[r])))          (fp32, three fused multiply-adds)
 * and 0 for rows j >= count[b].
 *
 * Point-to-plane step.  sh_align_plane_moments / sh_align_plane_moments_surface / sh_align_plane_solve are the Gauss-Newton
 * counterpart of the three calls above: the same pairs, kept rule, weights, ranges, grid and order (sh_align_ranges), but the
 * residual of a kept pair is measured along the unit normal at the model-side partner.  Everything below is fp64, every
 * operation rounded on its own (no contraction).  For a kept pair with p the (aligned) scan point (fp32, widened), q its
 * partner and nrm the normal there:
 *     r   = (nrm_0 (p_0 - q_0) + nrm_1 (p_1 - q_1)) + nrm_2 (p_2 - q_2)
 *     J   = [ nrm_0, nrm_1, nrm_2,  p_1 nrm_2 - p_2 nrm_1,  p_2 nrm_0 - p_0 nrm_2,  p_0 nrm_1 - p_1 nrm_0,
 *             (nrm_0 p_0 + nrm_1 p_1) + nrm_2 p_2 ]                                              (order: t, omega, sigma)
 * J is the derivative of r under the linearised increment p' = p + omega x p + sigma p + t.  Partner and normal:
 *     scan -> model, surface form:  q = the foot point of sh_align_moments_surface, unchanged; nrm = the normal of the recorded
 *         face: ab = b - a, ac = c - a, c = (cx, cy, cz) the fp32 cross product of "Vertex normals" (fma(u, v, -(w * z))), then
 *         fp64 len = sqrt((cx cx + cy cy) + cz cz), nrm = c / len (three divisions), the zero vector unless 0 < len < +inf
 *     scan -> model, vertex form:   q = x[idx_sm[j]], nrm = tn[idx_sm[j]]
 *     model -> scan, both forms:    q = x_i, p = s[idx_ms[i]], nrm = tn[i]
 * tn fp32 contiguous [B][n][3] as sh_vertex_normals writes it (may be NULL for the surface form with w_ms == 0).  A zero
 * normal contributes zeros to every sum; the pair still counts as kept.  partials: fp64
 * [B][sh_align_ranges(M, n, w_ms)][SH_ALIGN_PLANE_PARTIAL], per range the UNWEIGHTED sums
 *     [0] pairs kept  [1..28] sum J J^T, the upper triangle row-major ((0,0) (0,1) .. (0,6) (1,1) .. (6,6))  [29..35] sum J r
 *     [36] sum r^2  [37] active vertices of the range (model -> scan ranges only)
 * every element stored (a range beyond m_b holds zeros); thread t takes t, t + 256, ... of its range, then the fixed tree of
 * sh_align_moments.  One kernel template serves both calls.
 *
 * sh_align_plane_solve.  One wave per body.  The ranges' sums are added in range order per direction and joined with the
 * weights of sh_align_solve (1 / m_b, w_ms / n_act) into the system, sys fp64 [B][SH_ALIGN_PLANE_SYSTEM] (optional output):
 *     [0] W = sum w  [1..28] H = sum w J J^T (upper triangle)  [29..35] g = sum w J r  [36] sum w r^2
 * Lane 0 takes the leading k x k block, k = 3 (SH_ALIGN_TRANSLATION: t), 6 (SH_ALIGN_RIGID: t, omega) or 7; d_i = H_ii;
 * Hs_ij = H_ij / (sqrt(d_i) sqrt(d_j)) (unit diagonal), gs_i = g_i / sqrt(d_i); Cholesky Hs = L L^T column by column with the
 * pivot piv_j = Hs_jj - sum_{c<j} L_jc^2 (sums in ascending c), L_jj = sqrt(piv_j), L_ij = (Hs_ij - sum_{c<j} L_ic L_jc) / L_jj;
 * L y = -gs, L^T z = y, delta_i = z_i / sqrt(d_i), delta_i = 0 for i >= k.  Fixed loop counts, no data-dependent branch.  Then
 * c = exp(sigma); R = I + a K + b K^2 with K the cross-product matrix of omega, th2 = |omega|^2, a = sin(th) / th and
 * b = (1 - cos(th)) / th2, or a = 1 - th2 / 6, b = 1/2 - th2 / 24 when th2 < 1e-8; t = delta_t.  The pose so far is composed
 * with (c R, t) exactly as sh_align_solve composes, each value rounded to fp32 once, into pose_out / scale_out (may alias the
 * inputs).  solved int32 [B]: 1, or 0 when W == 0, a d_i (i < k) is not positive and finite, a pivot is not >
 * SH_ALIGN_PLANE_PIVOT_MIN (the block is singular to fp64 working precision: planar or parallel normals, too few pairs) or a
 * delta_i is not finite - then the increment is the identity, bitwise, and the pose passes through.  The step is Gauss-Newton:
 * it minimises the linearised sum w (r + J delta)^2, so the true weighted residual is not guaranteed to fall.  M, n, s_count
 * and w_ms must be those of the moments call.
 *
 * All of them: B == 0 is SH_OK with nothing launched; null pointers and negative sizes are SH_ERR_INVALID_ARG before the device
 * is touched; nothing allocates or synchronises.
 */
enum sh_align_mode { SH_ALIGN_TRANSLATION = 0, SH_ALIGN_RIGID = 1, SH_ALIGN_SIMILARITY = 2 };
#define SH_ALIGN_RANGE 2048
#define SH_ALIGN_PARTIAL 19
#define SH_ALIGN_MOMENTS 20
#define SH_ALIGN_JACOBI_SWEEPS 12
SH_API int sh_align_ranges(int M, int n, float w_ms);
SH_API size_t sh_align_partials_bytes(int B, int M, int n, float w_ms);
SH_API int sh_align_moments(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb, int rows, int n,
                            const uint8_t* v_mask, int64_t mask_sb, const int32_t* idx_sm, const float* d2_sm, const int32_t* idx_ms,
                            const float* d2_ms, float tau2, float w_ms, int B, double* partials, size_t partials_bytes,
                            sh_stream_t stream);
SH_API int sh_align_moments_surface(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb, int rows,
                                    int n, const uint8_t* v_mask, int64_t mask_sb, const int32_t* faces, int nF, const int32_t* face,
                                    const float* uv, const float* d2, const int32_t* idx_ms, const float* d2_ms, float tau2, float w_ms,
                                    int B, double* partials, size_t partials_bytes, sh_stream_t stream);
SH_API int sh_align_solve(const double* partials, int M, int n, const int32_t* s_count, float w_ms, int mode, int B,
                          const float* pose_in, const float* scale_in, float* pose_out, float* scale_out, float* inc, double* mom,
                          sh_stream_t stream);
SH_API int sh_transform_points(const float* src, int64_t src_sb, int M, const int32_t* count, const float* pose, int B, float* dst,
                               sh_stream_t stream);
#define SH_ALIGN_PLANE_PARTIAL 38
#define SH_ALIGN_PLANE_SYSTEM 37
#define SH_ALIGN_PLANE_PIVOT_MIN 1e-12
SH_API size_t sh_align_plane_partials_bytes(int B, int M, int n, float w_ms);
SH_API int sh_align_plane_moments(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb, int rows,
                                  int n, const uint8_t* v_mask, int64_t mask_sb, const float* tn, const int32_t* idx_sm,
                                  const float* d2_sm, const int32_t* idx_ms, const float* d2_ms, float tau2, float w_ms, int B,
                                  double* partials, size_t partials_bytes, sh_stream_t stream);
SH_API int sh_align_plane_moments_surface(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb,
                                          int rows, int n, const uint8_t* v_mask, int64_t mask_sb, const float* tn,
                                          const int32_t* faces, int nF, const int32_t* face, const float* uv, const float* d2,
                                          const int32_t* idx_ms, const float* d2_ms, float tau2, float w_ms, int B, double* partials,
                                          size_t partials_bytes, sh_stream_t stream);
SH_API int sh_align_plane_solve(const double* partials, int M, int n, const int32_t* s_count, float w_ms, int mode, int B,
                                const float* pose_in, const float* scale_in, float* pose_out, float* scale_out, double* sys,
                                int32_t* solved, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Robust terms: a robust penalty in the data term of the Chamfer loss and the matching IRLS weight in the pose steps (no
 * reference counterpart).  Two numbers select it: robust (enum sh_robust) and scale2 = sigma^2 > 0, sigma in the model's
 * normalised units.  The `_robust` entry points below take the arguments of their namesakes followed by (robust, scale2);
 * robust = SH_ROBUST_NONE is the namesake itself - the same kernels under the same names, the same bits, scale2 unread - and
 * the namesakes are that call.  An unknown robust, or with robust != SH_ROBUST_NONE a scale2 that is not finite and > 0:
 * SH_ERR_INVALID_ARG before anything else is looked at.
 *
 * The penalty applies to a pair's squared distance AFTER truncation: u = fminf(d2, tau2) for the value, and the kept rule
 * d2 < tau2 of the gradient and the moments is unchanged (there u = d2), so tau2 keeps its meaning and a point without a partner
 * (d2 = +inf under a gate) still counts as truncated.  Everything fp32, every operation rounded on its own (no contraction),
 * division and square root correctly rounded:
 *     SH_ROBUST_GEMAN_MCCLURE   t = scale2 / (scale2 + u);   rho = u * t;   w = t * t
 *     SH_ROBUST_HUBER           u <= scale2:  rho = u,  w = 1
 *       (on the distance)       otherwise:    rho = 2 * sqrtf(scale2 * u) - scale2,   w = sqrtf(scale2 / u)
 *                               as selects: rho = u <= scale2 ? u : r, w = u <= scale2 ? 1 : sqrtf(scale2 / (u <= scale2 ? 1 : u)),
 *                               so u = 0 never reaches the division
 * w = d rho / d u.  Both reduce to rho = u, w = 1 for u << scale2 and are continuous, with a continuous weight, across
 * u = scale2 (Huber: rho = scale2, w = 1 on both sides; Geman-McClure: rho = scale2 / 2, w = 1 / 4).  Geman-McClure is bounded
 * by scale2 and its weight falls as 1 / u^2: far points stop pulling.  Huber grows like the distance and its pull is constant.
 * u = +inf (no partner and no truncation) makes Geman-McClure's value NaN (inf * 0), where the plain value is +inf.
 *
 * sh_chamfer_fwd_robust.  L[b] of sh_chamfer_fwd with rho(min(d2, tau2)) in place of min(d2, tau2) in both sums: the same
 * normalisation (1 / m_b, w_ms / n_act), the terms widened to fp64 and summed in the same order.  counts as ever.
 *
 * sh_chamfer_bwd_robust, sh_chamfer_surface_bwd_robust.  The gradient of that value, w taken from the recorded fp32 d2 of the
 * pair: a kept pair contributes w * 2 (x - s) in place of 2 (x - s).
 *     vertex partner:   acc = fma(w(d2_sm[j]), fl(x_i - s_j), acc) per coordinate, ascending j           (fp32)
 *     surface partner:  e = fl(w(d2[j]) * e) per coordinate, once per pair, before the corners' l_k; the rest as ever
 *     model -> scan:    the factor (w_ms 2/n_act) becomes fl((w_ms 2/n_act) * w(d2_ms[i])), both forms
 * The kept rule, the order, the epilogue and the rows that receive zeros are those of the namesakes.
 *
 * sh_align_moments_robust, sh_align_moments_surface_robust, sh_align_plane_moments_robust,
 * sh_align_plane_moments_surface_robust.  One IRLS step: a kept pair adds w times what it adds in the namesake, w = the fp32
 * weight above of the pair's recorded d2 (d2_sm / the surface d2 / d2_ms), widened to fp64; the pair's terms are formed exactly
 * as in the namesake and each multiplied by w once before it is added.  Slot [0] of a range, "pairs kept", is therefore the sum
 * of the weights; the active-vertex slot stays a count.  Ranges, grid, order and the partials' layout do not change, and the
 * two solve calls finish these partials unchanged.  What every divisor of the solve kernels means under weights:
 *     1 / m_b and w_ms / n_act    the two directions' normalisation: counts of points and of active vertices, as in the value -
 *                                 not pair counts, so they stay counts
 *     1 / W (sh_align_solve)      W = sum of the joined weights (direction weight times w): p_bar, q_bar, H and var_p are the
 *                                 weighted means and covariances, which is what weighted Procrustes asks for
 *     W > 0 / sy[0] > 0           "something was kept" - a sum of positive weights is positive whenever a pair was kept (w > 0
 *                                 for every finite u)
 *     mom[18]                     the sum of the two directions' slots [0]: the unnormalised sum of weights; with
 *                                 SH_ROBUST_NONE the pair count, as ever
 *     sh_align_plane_solve        divides by nothing of the kind: H and g carry the same factor
 * The weight is taken from the RECORDED d2 - the distance the search measured, which is also the distance the value's rho was
 * evaluated at - not recomputed from the pair: for a foot point or a gated match that is the only distance there is, and value,
 * gradient and pose step then weigh a pair alike.
 *
 * No atomics; the same bits for a body alone or in any padded batch.
 */
enum sh_robust { SH_ROBUST_NONE = 0, SH_ROBUST_GEMAN_MCCLURE = 1, SH_ROBUST_HUBER = 2 };
SH_API int sh_chamfer_fwd_robust(const float* d2_sm, int M, const int32_t* s_count, const float* d2_ms, int rows, int n,
                                 const uint8_t* v_mask, int64_t mask_sb, float tau2, float w_ms, int B, float* loss, int32_t* counts,
                                 sh_stream_t stream, int robust, float scale2);
SH_API int sh_chamfer_bwd_robust(const float* x, int64_t x_sb, int rows, int n, const float* s, int64_t s_sb, int M,
                                 const int32_t* s_count, const int32_t* idx_sm, const float* d2_sm, const int32_t* idx_ms,
                                 const float* d2_ms, const uint8_t* v_mask, int64_t mask_sb, const int32_t* counts, float tau2,
                                 float w_ms, const float* gL, int B, float* g_x, sh_stream_t stream, int robust, float scale2);
SH_API int sh_chamfer_surface_bwd_robust(const float* x, int64_t x_sb, int rows, int n, const float* s, int64_t s_sb, int M,
                                         const int32_t* s_count, const int32_t* faces, int nF, const int32_t* face, const float* d2,
                                         const float* uv, const int32_t* idx_ms, const float* d2_ms, const uint8_t* v_mask,
                                         int64_t mask_sb, const int32_t* counts, float tau2, float w_ms, const float* gL, int B,
                                         float* g_x, sh_stream_t stream, int robust, float scale2);
SH_API int sh_align_moments_robust(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb, int rows,
                                   int n, const uint8_t* v_mask, int64_t mask_sb, const int32_t* idx_sm, const float* d2_sm,
                                   const int32_t* idx_ms, const float* d2_ms, float tau2, float w_ms, int B, double* partials,
                                   size_t partials_bytes, sh_stream_t stream, int robust, float scale2);
SH_API int sh_align_moments_surface_robust(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb,
                                           int rows, int n, const uint8_t* v_mask, int64_t mask_sb, const int32_t* faces, int nF,
                                           const int32_t* face, const float* uv, const float* d2, const int32_t* idx_ms,
                                           const float* d2_ms, float tau2, float w_ms, int B, double* partials, size_t partials_bytes,
                                           sh_stream_t stream, int robust, float scale2);
SH_API int sh_align_plane_moments_robust(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb,
                                         int rows, int n, const uint8_t* v_mask, int64_t mask_sb, const float* tn, const int32_t* idx_sm,
                                         const float* d2_sm, const int32_t* idx_ms, const float* d2_ms, float tau2, float w_ms, int B,
                                         double* partials, size_t partials_bytes, sh_stream_t stream, int robust, float scale2);
SH_API int sh_align_plane_moments_surface_robust(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x,
                                                 int64_t x_sb, int rows, int n, const uint8_t* v_mask, int64_t mask_sb, const float* tn,
                                                 const int32_t* faces, int nF, const int32_t* face, const float* uv, const float* d2,
                                                 const int32_t* idx_ms, const float* d2_ms, float tau2, float w_ms, int B,
                                                 double* partials, size_t partials_bytes, sh_stream_t stream, int robust,
                                                 float scale2);

/* ---------------------------------------------------------------------------------------------
 * Depth images: a depth map as a scan - the camera-frame point of every usable pixel, its normal from the pixel grid, and the
 * rows packed per body in a fixed order (no reference counterpart).  Deterministic: no atomics of any kind, every output element
 * written by one plain store; the bits depend on neither batch, padding nor launch shape.
 *
 * Inputs.  depth: contiguous [B][H][W], fp32 (dtype SH_DEPTH_F32) or 16-bit unsigned words (SH_DEPTH_U16, raw sensor units; a
 * buffer of int16 is read as unsigned).  intr: fp32 [B][4] = (fx, fy, cx, cy) per body, pinhole, no distortion.  mask: uint8
 * [B][H][W] or NULL, 0 = "not the subject".  z_near, z_far: the accepted range (-inf / +inf: none).  max_step: the largest depth
 * difference between grid neighbours of one surface (+inf: none).  stride >= 1.  Pixel (u, v): column u, row v.
 * Everything below is fp32 with every operation rounded on its own (no contraction) and a correctly rounded division, except
 * the normal, which is fp64 as marked.
 *     z      = fl((float)raw * depth_scale)                                         (both input types)
 *     valid  iff z is finite and z > 0, z_near <= z <= z_far, raw != 0 for 16-bit input, and mask != 0 where a mask is given
 *     X = fl(fl(fl((float)u - cx) * z) / fx);   Y = fl(fl(fl((float)v - cy) * z) / fy);   Z = z;      P = (X, Y, Z)
 * The frame is the camera's; the viewpoint is the origin.
 * Usable neighbour of pixel c: inside the image, valid, and fabsf(z_nb - z_c) <= max_step.  A depth step between neighbours is
 * what a silhouette (and a flying pixel on it) looks like: no tangent crosses one.
 * Tangents, differences component-wise in fp32.  Horizontal, over L = (u - 1, v) and R = (u + 1, v):
 *     dx = P_R - P_L  when both are usable;  else P_R - P_c;  else P_c - P_L;  else none
 * vertical dy by the same rule over (u, v - 1) and (u, v + 1).  Tangents always read the full-resolution neighbours, whatever the
 * stride.
 * Normal, fp64: the components of dx, dy and P_c widened, products of two such values exact.
 *     c    = dx x dy       each component one rounded subtraction of two exact products
 *     len2 = (c_x c_x + c_y c_y) + c_z c_z
 *     unknown - a row of exact zeros, as everywhere in this library - when a tangent is missing or !(len2 > 0)
 *     n    = c / sqrt(len2), negated when (c_x X + c_y Y) + c_z Z > 0 (it then points away from the camera), each component
 *            rounded to fp32 once
 * Kept: valid, u % stride == 0 and v % stride == 0, and - when drop_isolated != 0 - the normal is known.
 * Order of the kept rows, part of the contract: SH_DEPTH_TILE x SH_DEPTH_TILE pixel tiles in row-major tile order; inside a
 * tile the Z-order of (u & 15, v & 15): bit k of u is bit 2k of the rank, bit k of v bit 2k + 1.  Tile order on the image is a
 * space-filling order on the surface - what the surface search's cull lives on.
 *
 * sh_depth_count -> counts int32 [B], the kept pixels per body, and in `workspace` (sh_depth_workspace(B, H, W) bytes, int32
 * [B][tiles]) the first row of every tile.  sh_depth_points, given the same inputs, that workspace, the counts and a width
 * M >= max_count (the largest count, as the caller read it), -> points fp32 [B][M][3], normals fp32 [B][M][3], pixel int32 [B][M]
 * = v * W + u; rows at or beyond a body's count hold zeros in points and normals and -1 in pixel.  No row >= M is ever written.
 *
 * How it is computed.  One workgroup of 256 threads per tile, thread = Z-rank: the 18 x 18 tile with its halo goes into LDS in
 * coalesced rows as z (NaN where not valid, so that one compare decides "usable"), and the five points are formed from LDS.
 * (1) The count pass: a wave ballot of "kept", popcount, the four wave totals combined through LDS -> the tile's count.  (2) A
 * per-body exclusive scan of the tile counts, one workgroup per body looping over the tiles, in place; it also writes counts.
 * (3) The emit pass recomputes the pixel; its row is the tile's first row plus its rank among the tile's kept pixels from the
 * ballot prefix; the workgroups of a body also share out the padding rows.  Memory-bound: the depth (and mask) is read twice,
 * every output written once.
 * B == 0 or H * W == 0: SH_OK, nothing launched.  Null pointers (mask excepted), negative sizes, stride < 1, M < max_count or an
 * unknown dtype: SH_ERR_INVALID_ARG before the device is touched; a workspace that is too small: SH_ERR_WORKSPACE.
 */
enum sh_depth_dtype { SH_DEPTH_F32 = 0, SH_DEPTH_U16 = 1 };
#define SH_DEPTH_TILE 16
SH_API size_t sh_depth_workspace(int B, int H, int W);
SH_API int sh_depth_count(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, int B, int H, int W,
                          float z_near, float z_far, float max_step, int drop_isolated, int stride, int32_t* counts, void* workspace,
                          size_t workspace_bytes, sh_stream_t stream);
SH_API int sh_depth_points(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, int B, int H, int W,
                           float z_near, float z_far, float max_step, int drop_isolated, int stride, const int32_t* counts,
                           int max_count, int M, const void* workspace, size_t workspace_bytes, float* points, float* normals,
                           int32_t* pixel, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Depth views: the V calibrated depth cameras of a rig as ONE scan per body, in the rig's frame (no reference counterpart).
 * Deterministic as "Depth images": no atomics, every output element one plain store, bits independent of B, of the padding and
 * of the other bodies.
 *
 * Inputs.  depth [B][V][H][W], intr fp32 [B][V][4], mask uint8 [B][V][H][W] or NULL: per image as in "Depth images", with its
 * dtype / depth_scale / z_near / z_far / max_step / drop_isolated / stride.  ext: fp32 [B][V][12], camera frame -> rig frame in
 * the layout of sh_transform_points - R row-major (r_00 .. r_22), then t - and rigid (R a proper rotation, no scale; the caller's
 * duty).  1 <= V <= SH_DEPTH_MAX_VIEWS.  A view whose ext row holds a NaN is ABSENT: it emits no row, its counts are 0, and
 * nothing else of it - depth, mask, intrinsics - is read.
 * Per pixel, everything up to the camera-frame point P = (X, Y, Z) and the fp64 unit normal n (after its flip towards the
 * camera, BEFORE its rounding) is "Depth images", unchanged.  Then, with no contraction:
 *     P'_i = fl(fl(fl(fl(r_i0 * X) + fl(r_i1 * Y)) + fl(r_i2 * Z)) + t_i)        fp32, i = 0..2
 *     n'_i = (r_i0 * n_x + r_i1 * n_y) + r_i2 * n_z                              fp64: R widened; each component rounded to fp32
 *                                                                                once (this replaces the rounding of n)
 *     an unknown normal (a zero row) stays a zero row
 * Order.  Within a body view-major; inside a view the tile / Z-order of "Depth images".
 *
 * sh_depth_views_count -> counts int32 [B], the kept pixels of a body over all its views, and in `workspace`
 * (sh_depth_views_workspace(B, V, H, W) bytes, int32 [B][V][tiles]) the first row of every tile.  sh_depth_views_points, given
 * the same inputs, that workspace, the counts and a width M >= max_count, -> points fp32 [B][M][3] = P', normals fp32 [B][M][3] =
 * n', pixel int32 [B][M] = v * W + u within the row's own view, view uint8 [B][M], and view_first int32 [B][V + 1]: the first
 * row of each view, the last entry the count (an empty or absent view repeats its successor's).  Rows at or beyond a body's
 * count hold zeros, zeros, -1 and 255.  No row >= M is ever written.
 *
 * How it is computed.  The three passes of "Depth images" with image = body * V + view: the count pass over B V images, ONE
 * exclusive scan per body over its V * tiles tile counts, and the emit pass, which applies the transform and shares the body's
 * padding out over the workgroups of all its views.
 * B == 0 or H * W == 0: SH_OK, nothing launched (view_first is not written).  Null pointers (mask excepted), V outside
 * [1, SH_DEPTH_MAX_VIEWS], negative sizes, stride < 1, M < max_count or an unknown dtype: SH_ERR_INVALID_ARG before the device is
 * touched; a workspace that is too small: SH_ERR_WORKSPACE; B * V > 65535 or V * H * W > INT_MAX: SH_ERR_UNSUPPORTED.
 */
#define SH_DEPTH_MAX_VIEWS 32
SH_API size_t sh_depth_views_workspace(int B, int V, int H, int W);
SH_API int sh_depth_views_count(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, const float* ext,
                                int B, int V, int H, int W, float z_near, float z_far, float max_step, int drop_isolated, int stride,
                                int32_t* counts, void* workspace, size_t workspace_bytes, sh_stream_t stream);
SH_API int sh_depth_views_points(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, const float* ext,
                                 int B, int V, int H, int W, float z_near, float z_far, float max_step, int drop_isolated, int stride,
                                 const int32_t* counts, int max_count, int M, const void* workspace, size_t workspace_bytes, float* points,
                                 float* normals, int32_t* pixel, uint8_t* view, int32_t* view_first, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Depth views: overlap - which rows of a rig's fused scan another, better-placed camera also measures (no reference counterpart).
 * Projective data association: no search, O(M V) work, one scattered read of the depth images.  Deterministic: no atomics, every
 * output element one plain store, bits independent of B, of the padding and of the launch shape.
 *
 * Inputs.  depth, dtype, depth_scale, intr, mask, ext, B, V, H, W, z_near, z_far: exactly those of sh_depth_views_points, and the
 * packed rows that call produced: points fp32 [B][M][3], normals fp32 [B][M][3], view uint8 [B][M], counts int32 [B].  tol fp32
 * >= 0 (+inf: any depth agrees).  max_step, drop_isolated and stride are not consulted.
 * Everything is fp32, every operation rounded on its own (no contraction), the division correctly rounded; no square root.
 * For a live row (row < counts[b]) with point P, normal n and own view a, every view c that is not absent (a NaN in its ext row):
 *     e    = t_c - P                                                    component-wise
 *     len2 = fl(fl(fl(e_x e_x) + fl(e_y e_y)) + fl(e_z e_z))
 *     dot  = fl(fl(fl(n_x e_x) + fl(n_y e_y)) + fl(n_z e_z))
 *     q_c  = fl(fl(dot * fabsf(dot)) / fl(fl(len2 * len2) * len2)),  0 when len2 == 0
 * - cos^2(theta) / d^4 with the sign of the cosine, monotone in cos(theta) / d^2, what depth noise shrinks with - evaluated with the
 * row's OWN normal (the same surface point has the same normal whoever looks at it), for c == a by the same expression; an
 * unknown normal (a zero row) gives q = 0 for every view.  For c != a, with d = P - t_c:
 *     Q_j  = fl(fl(fl(r_0j d_0) + fl(r_1j d_1)) + fl(r_2j d_2))         Q = R_c^T d, the point in c's camera frame
 *     !(Q_z > 0) (a NaN included): c does not observe the row.  Else (uf, vf), "inside" and the nearest pixel (u, v) from
 *     (Q_x, Q_y, Q_z) and view c's intrinsics exactly as sh_free_space_fwd forms them from (X, Y, Z); not inside: not observed
 *     z_c  = fl((float)raw * depth_scale) at pixel (u, v) of image (b, c)
 *     c OBSERVES the row iff that pixel is valid in the sense of "Depth images" (one set of device helpers serves all) and
 *     fabsf(fl(z_c - Q_z)) <= tol
 * Outputs.  seen uint32 [B][M]: bit c set iff c observes the row; bit a is always set for a live row.  keep uint8 [B][M]: 0 iff
 * some observing c != a has q_c > q_a, or q_c == q_a and c < a (of two identical cameras the first survives); else 1.  Padding
 * rows (row >= counts[b]) get 0 in both.
 * How it is computed.  One launch, grid (256-row chunk, body), one thread per row; the body's V extrinsics and intrinsics are
 * staged in LDS once per workgroup, the loop over the views is uniform.
 * Null pointers (mask excepted), V outside [1, SH_DEPTH_MAX_VIEWS], negative sizes, an unknown dtype, tol negative or NaN:
 * SH_ERR_INVALID_ARG; B > 65535, B * V > 65535 or V * H * W > INT_MAX: SH_ERR_UNSUPPORTED; all before the device is touched.
 * B == 0 or M == 0: SH_OK, nothing launched.
 *
 * Scan compaction: sh_scan_compact, a stable per-body compaction of a rig's rows under a keep plane, out of place.  Inputs: points,
 * normals fp32 [B][M][3], pixel int32 [B][M], view uint8 [B][M] (ascending within a body: view-major rows), seen uint32 [B][M] or
 * NULL (then seen_out is NULL too), keep uint8 [B][M], counts int32 [B], V, and a width M_out >= max_kept, the largest kept
 * count as the caller read it.  A row is kept iff row < counts[b] and keep != 0.
 * Outputs: the same arrays at width M_out with the kept rows in their old order, the padding zeros, zeros, -1, 255 and 0;
 * counts_out int32 [B]; view_first_out int32 [B][V + 1] with the meaning of "Depth views".  No row >= M_out is ever written.  No
 * atomics; the same bits for a body alone and in any batch.
 * How it is computed.  The three passes of "Depth images" over 256-row chunks: a count pass (ballot, popcount, four wave totals),
 * the same per-body exclusive scan kernel (it writes counts_out), and an emit pass - output row = the chunk's first row + the
 * ballot rank; view_first_out is written by the rows at which `view` steps and by the last live row.  `workspace`
 * (sh_scan_compact_workspace(B, M) bytes, int32 [B][chunks]) holds the chunk rows.
 * Null pointers (seen excepted), V outside [1, SH_DEPTH_MAX_VIEWS], negative sizes, M_out < max_kept, an output that is its
 * input: SH_ERR_INVALID_ARG; B > 65535: SH_ERR_UNSUPPORTED; a workspace that is too small: SH_ERR_WORKSPACE; before the device
 * is touched.  B == 0: SH_OK, nothing launched; M == 0 still writes the padding, counts_out and view_first_out (zeros).
 */
SH_API int sh_depth_views_overlap(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, const float* ext,
                                  int B, int V, int H, int W, float z_near, float z_far, const float* points, const float* normals,
                                  const uint8_t* view, const int32_t* counts, int M, float tol, uint32_t* seen, uint8_t* keep,
                                  sh_stream_t stream);
SH_API size_t sh_scan_compact_workspace(int B, int M);
SH_API int sh_scan_compact(const float* points, const float* normals, const int32_t* pixel, const uint8_t* view, const uint32_t* seen,
                           const uint8_t* keep, const int32_t* counts, int B, int V, int M, int max_kept, int M_out, void* workspace,
                           size_t workspace_bytes, float* points_out, float* normals_out, int32_t* pixel_out, uint8_t* view_out,
                           uint32_t* seen_out, int32_t* counts_out, int32_t* view_first_out, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Depth field: what a depth image says about where the body is NOT - the way back from the model to the image (no reference
 * counterpart).  A packing-time field per image (sh_depth_field) and a per-step vertex term with its gradient
 * (sh_free_space_fwd / _bwd).  Deterministic: no atomics of any kind, every output element written by one plain store; the bits
 * depend on neither batch nor launch shape.
 *
 * sh_depth_field.  Inputs: those of sh_depth_count - depth, dtype, depth_scale, intr, mask, z_near, z_far, with the same
 * z = fl((float)raw * depth_scale) and the same "valid" (one set of device helpers serves both).  intr is not read: the field is
 * a function of the image alone; it is taken so that the two calls have one argument list.  Per pixel three planes:
 *     cls uint8 [B][H][W]     SH_FIELD_SURFACE (2): valid in the sense of "Depth images".
 *                             SH_FIELD_EMPTY (0): there is a reading (z finite and positive, the word not 0), the pixel is not
 *                             SURFACE, and z >= z_near - the sensor saw past the working volume, or the mask says "not the
 *                             subject" at a depth that cannot occlude it.
 *                             SH_FIELD_UNKNOWN (1): everything else - no reading, or something nearer than z_near, behind which
 *                             the body may be.
 *     z fp32 [B][H][W]        the depth of a SURFACE pixel, 0 elsewhere
 *     nearest int32 [B][H][W] the exact feature transform of the ALLOWED set, allowed = cls != 0: the index v' * W + u' of the
 *                             allowed pixel that minimises the integer (u - u')^2 + (v - v')^2; ties go to the smallest index;
 *                             an allowed pixel is its own nearest; -1 when the image has no allowed pixel.
 * nearest is a pure function of cls: the same bits for an image alone and in any batch.
 * How it is computed.  (1) The column pass, one thread per column (coalesced across u): down the column it classifies and
 * records the row of the nearest allowed pixel at or above, up again the nearest at or below, and keeps the closer of the two, a
 * tie going to the upper (the smaller index) - one candidate row per (pixel, column), int16 in `workspace`
 * (sh_depth_field_workspace(B, H, W) bytes), -1 for a column with no allowed pixel.  One candidate is enough: within a column d2
 * and the index grow together.  (2) The row pass, one workgroup per image row with the row's W candidates in LDS (2 W bytes, at
 * most 32 KiB: never chunked): a pixel walks outward from its own column, k = 0, 1, ..., takes the minimum of the key
 * (d2, v' * W + u') over columns u - k and u + k, and leaves once k * k > its best d2 (at k * k == best a tie of smaller index is
 * still possible).  The walk is as long as the distance to the nearest allowed pixel; an image without one walks every row whole.
 * H or W above SH_FIELD_MAX_SIDE (d2 must fit in 31 bits, a row in int16) or B > 65535: SH_ERR_UNSUPPORTED.  Null pointers (mask
 * excepted), negative sizes, an unknown dtype and a workspace that is too small: SH_ERR_INVALID_ARG.  All of that before the
 * device is touched.  B == 0 or H * W == 0: SH_OK, nothing launched.
 *
 * sh_free_space_fwd / sh_free_space_bwd.  x: fp32 [B] bodies of CAMERA-frame points, batch stride x_sb; the first n of `rows`
 * rows are vertices, rows >= n are never read and get zero gradient.  v_mask [n] (mask_sb = 0) or [B][n] (mask_sb = n), NULL: all
 * active.  margin fp32 >= 0.  cls, z, nearest: a field of the same B, H, W; intr [B][4] = (fx, fy, cx, cy).  Everything is fp32
 * with every operation rounded on its own (no contraction) and a correctly rounded division.  For an active vertex (X, Y, Z):
 *     kind SH_FS_OUTSIDE (4), no term:   !(Z > 0) (a NaN included), or (uf, vf) below not inside
 *     uf = fl(fl(fl(X * fx) / Z) + cx);  vf = fl(fl(fl(Y * fy) / Z) + cy)
 *     inside: uf >= -0.5f, uf < W - 0.5f, vf >= -0.5f, vf < H - 0.5f                                    (a NaN is outside)
 *     u = (int)floorf(fl(uf + 0.5f));  v = (int)floorf(fl(vf + 0.5f));  c = cls[b][v][u]              (nearest-pixel sampling)
 *     c == 1:  kind SH_FS_UNKNOWN (3), no term
 *     c == 2:  e = fl(fl(z[b][v][u] - margin) - Z);  e > 0: kind SH_FS_FREE (1), term = fl(e * e), g = (0, 0, fl(-2 * e));
 *              else kind SH_FS_NONE (0), no term
 *     c == 0:  q = nearest[b][v][u];  q < 0: kind 0, no term.  Else (uq, vq) = (q % W, q / W),
 *              a = fl(fl((float)uq - cx) / fx),  b = fl(fl((float)vq - cy) / fy),
 *              rx = fl(X - fl(a * Z)),  ry = fl(Y - fl(b * Z))     (the vertex's offset from the ray through that pixel, at its
 *              own depth);  kind SH_FS_SILHOUETTE (2), term = fl(fl(rx * rx) + fl(ry * ry)),
 *              g = (fl(2 * rx), fl(2 * ry), fl(-2 * fl(fl(a * rx) + fl(b * ry))))
 * nearest is taken as a constant, as the Chamfer gradient takes its indices; so is the image: there is no image gradient.  A
 * masked vertex has kind 0, no term and no gradient.
 * sh_free_space_fwd -> term fp32 [B][n] (0 where there is none), kind uint8 [B][n], loss fp32 [B][2] = (1 / n_act) * the sum of
 * the terms of kind 1 and of kind 2 (n_act = the active vertices; sums in fp64 in the order of sh_chamfer_fwd: thread t of 256
 * takes vertices t, t + 256, ..., then the wave butterfly and the four wave sums in order; one rounding to fp32; n_act == 0:
 * zeros), counts int32 [B][4] = (n_act, #kind 1, #kind 2, #kind 4).  One launch, one workgroup per body.
 * sh_free_space_bwd, given the forward call's arguments, its counts and gL fp32 [B][2] -> g_x fp32 [B][rows][3], contiguous:
 *     g_x[b][i] = fl(fl(gL[b][k] * fl(1 / (float)n_act)) * g)  per component, k = 0 for kind 1 and 1 for kind 2
 * and zeros in every other row below `rows`.  One launch, one thread per row; the vertex's case list is evaluated again.
 * Both run the kernels of "Free space from a rig" below as a rig of one camera WITHOUT a cam: the vertex is taken as it is and the
 * gradient handed back as it is, with no products - under an identity cam 0 * inf would turn a vertex at Z = +inf into kind 4
 * and -0 + 0 would lose the sign of a zero gradient word.  At V = 1 the layouts and the order of the sums there are the ones above.
 * Null pointers (v_mask excepted), negative sizes, n > rows, a batch or mask stride shorter than n, a negative or NaN margin,
 * H * W == 0 with n > 0: SH_ERR_INVALID_ARG; H or W above SH_FIELD_MAX_SIDE: SH_ERR_UNSUPPORTED; before the device is touched.
 * B == 0: SH_OK, nothing launched.
 */
enum sh_field_class { SH_FIELD_EMPTY = 0, SH_FIELD_UNKNOWN = 1, SH_FIELD_SURFACE = 2 };
enum sh_free_space_kind { SH_FS_NONE = 0, SH_FS_FREE = 1, SH_FS_SILHOUETTE = 2, SH_FS_UNKNOWN = 3, SH_FS_OUTSIDE = 4 };
#define SH_FIELD_MAX_SIDE 16384
SH_API size_t sh_depth_field_workspace(int B, int H, int W);
SH_API int sh_depth_field(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, int B, int H, int W,
                          float z_near, float z_far, uint8_t* cls, float* z, int32_t* nearest, void* workspace, size_t workspace_bytes,
                          sh_stream_t stream);
SH_API int sh_free_space_fwd(const float* x, int64_t x_sb, int rows, int n, const uint8_t* cls, const float* z, const int32_t* nearest,
                             const float* intr, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin, int B, float* term,
                             uint8_t* kind, float* loss, int32_t* counts, sh_stream_t stream);
SH_API int sh_free_space_bwd(const float* x, int64_t x_sb, int rows, int n, const uint8_t* cls, const float* z, const int32_t* nearest,
                             const float* intr, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin, const int32_t* counts,
                             const float* gL, int B, float* g_x, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Free space from a rig: the term of "Depth field" for the V calibrated cameras of "Depth views" at once, with the way from the
 * model's frame into each camera's frame inside the kernels (no reference counterpart).  Deterministic: no atomics, every output
 * element written by one plain store; the bits depend on neither B, the padding nor the launch shape.  fp32 operations are
 * rounded one at a time (no contraction), fp64 ones too; every division is correctly rounded.  1 <= V <= SH_DEPTH_MAX_VIEWS.
 *
 * sh_free_space_cameras.  pose: fp32 [B][12], scan / rig frame -> model frame, A row-major (a_00 .. a_22) then t (the layout of
 * sh_transform_points), or NULL: the identity.  ext: fp32 [B][V][12], camera frame -> rig frame, R row-major then t_v ("Depth
 * views").  -> cam fp32 [B][V][12] = (M | c), model frame -> camera frame, q = M x + c, M row-major (m_00 .. m_22) then c:
 *     M = R^T A^-1,   c = -R^T (A^-1 t + t_v)
 * in fp64 from the widened inputs, in this order, with a_i the rows of A:
 *     k_0 = a_1 x a_2,  k_1 = a_2 x a_0,  k_2 = a_0 x a_1      (p x q)_0 = p_1 q_2 - p_2 q_1, and cyclically: two products, one difference
 *     det = (a_00 k_00 + a_01 k_01) + a_02 k_02
 *     I_ij = k_ji / det                                          A^-1 by the adjugate; nothing is rounded to fp32 in between
 *     p_i  = ((I_i0 t_0 + I_i1 t_1) + I_i2 t_2) + t_v,i
 *     M_ij = (r_0i I_0j + r_1i I_1j) + r_2i I_2j
 *     c_i  = -((r_0i p_0 + r_1i p_1) + r_2i p_2)
 * and each of the 12 words rounded to fp32 once.  An ext row that holds a NaN (an ABSENT camera, "Depth views"), or a body whose
 * det is 0 or not finite, gives 12 NaN words.  One launch, one thread per (body, view).
 *
 * sh_free_space_views_fwd / _bwd.  x, x_sb, rows, n, v_mask, mask_sb, margin: those of sh_free_space_fwd, but x holds points of
 * the MODEL's frame (any frame cam starts from).  cam fp32 [B][V][12]; intr fp32 [B][V][4]; cls, z, nearest [B][V][H][W]: image
 * (b, v) is image b * V + v of an sh_depth_field call over B * V images.  For an active vertex x and every view v, ascending:
 *     Q_i = fl(fl(fl(fl(m_i0 * x_0) + fl(m_i1 * x_1)) + fl(m_i2 * x_2)) + c_i)                          i = 0..2, the form of "Depth views"
 * and then the case list of sh_free_space_fwd, unchanged, on (X, Y, Z) = Q with view v's intrinsics and image (one device
 * routine serves both).  A NaN cam row gives kind SH_FS_OUTSIDE by !(Z > 0), and nothing of that view's image is read.  With an
 * identity cam row Q == x for finite x.
 * sh_free_space_views_fwd -> term fp32 [B][V][n], kind uint8 [B][V][n] (a masked vertex: 0 and kind 0 in every view), loss fp32
 * [B][2] = (1 / n_act) * the sum over vertices AND views of the kind-1 terms, and of the kind-2 terms; counts int32 [B][V][4] =
 * (n_act, #kind 1, #kind 2, #kind 4) per view (n_act is the same in every view).  The sums are fp64, in this order: thread t of
 * 256 takes the vertices t, t + 256, ... in order and, inside a vertex, the views ascending; then the wave butterfly and the four
 * wave sums in order; one division by n_act and one rounding to fp32 (n_act == 0: zeros).  One launch, one workgroup per body:
 * all its threads write term and kind, one thread per vertex with a uniform loop over the views; after a barrier the first 256
 * fold the stored terms in the order above - so the order, not the workgroup's width, makes the bits.
 * sh_free_space_views_bwd, given the forward call's arguments, its counts and gL fp32 [B][2] -> g_x fp32 [B][rows][3],
 * contiguous.  Per row, starting from (0, 0, 0) and for the views ascending that gave the vertex a term of kind k + 1:
 *     w_i     = fl(fl(gL[b][k] * fl(1 / (float)n_act)) * g_i)                                         g: the camera-frame gradient of the case list
 *     g_x[j] += fl(fl(fl(m_0j * w_0) + fl(m_1j * w_1)) + fl(m_2j * w_2))                              M^T w, one fp32 addition per view
 * Rows without a term, masked rows and rows >= n hold zeros.  One launch, one thread per row, a uniform loop over the views.
 * In both term kernels the body's V records (12 cam words, 4 intrinsics) are staged in LDS once per workgroup.
 * In the library's launch records (and the profiles made from them) these two launches read free_space_views_fwd_kernel and
 * free_space_views_bwd_kernel: the entry point's name, not a symbol - the kernels are free_space_fwd_kernel<true> and
 * free_space_bwd_kernel<true>, the one-camera entry points launch the <false> instantiations.
 * Null pointers (v_mask, and pose for the cameras, excepted), V outside [1, SH_DEPTH_MAX_VIEWS], negative sizes, n > rows, a batch
 * or mask stride shorter than n, a negative or NaN margin, H * W == 0 with n > 0: SH_ERR_INVALID_ARG; H or W above
 * SH_FIELD_MAX_SIDE, B > 65535, B * V > 65535 or V * H * W > INT_MAX: SH_ERR_UNSUPPORTED; all before the device is touched.
 * B == 0: SH_OK, nothing launched.
 */
SH_API int sh_free_space_cameras(const float* pose, const float* ext, int B, int V, float* cam, sh_stream_t stream);
SH_API int sh_free_space_views_fwd(const float* x, int64_t x_sb, int rows, int n, const float* cam, const uint8_t* cls, const float* z,
                                   const int32_t* nearest, const float* intr, int V, int H, int W, const uint8_t* v_mask, int64_t mask_sb,
                                   float margin, int B, float* term, uint8_t* kind, float* loss, int32_t* counts, sh_stream_t stream);
SH_API int sh_free_space_views_bwd(const float* x, int64_t x_sb, int rows, int n, const float* cam, const uint8_t* cls, const float* z,
                                   const int32_t* nearest, const float* intr, int V, int H, int W, const uint8_t* v_mask, int64_t mask_sb,
                                   float margin, const int32_t* counts, const float* gL, int B, float* g_x, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Camera rays: lens distortion for the depth cameras of "Depth images", "Depth views", "Depth views: overlap" and "Free space from
 * a rig" (no reference counterpart).  A depth image cannot be rectified beforehand - resampling interpolates across depth steps -
 * so the lens lives inside the unprojection (pixel -> ray, a table made once per calibrated camera) and inside the projection
 * (point -> pixel, evaluated in the kernels).  Deterministic: no atomics, every output element one plain store, the same bits
 * for a camera alone and in any batch.
 *
 * The model is OpenCV's 8-coefficient rational one, d = (k1, k2, p1, p2, k3, k4, k5, k6) in that order, for the normalised point
 * (a, b) = (X / Z, Y / Z).  ONE order of operations, every operation rounded on its own (no contraction), every division
 * correctly rounded; T is fp32 in the forward model and fp64 in the inverse:
 *     a2 = a * a;  b2 = b * b;  r2 = a2 + b2;  r4 = r2 * r2;  r6 = r4 * r2
 *     num = ((1 + k1 * r2) + k2 * r4) + k3 * r6
 *     den = ((1 + k4 * r2) + k5 * r4) + k6 * r6
 *     ab = a * b
 *     tx = (2 * p1) * ab + p2 * (r2 + 2 * a2)
 *     ty = p1 * (r2 + 2 * b2) + (2 * p2) * ab
 *     rad = num / den
 *     ad = a * rad + tx;  bd = b * rad + ty
 *     u = fx * ad + cx;   v = fy * bd + cy
 *
 * Forward, point -> pixel, fp32, for Z > 0:  a = fl(X / Z), b = fl(Y / Z);  !(r2 <= limit) (a NaN included): the point is
 * OUTSIDE, whatever the polynomial would say - beyond the limit the model may fold back into the image; else (uf, vf) = (u, v)
 * above, and the inside test and the rounding to a pixel of sh_free_space_fwd follow unchanged.
 *
 * Inverse, pixel -> ray: sh_camera_rays(intr fp32 [C][4], dist fp32 [C][8], C, H, W) -> rays fp32 [C][H][W][2], limit fp32 [C],
 * complete int32 [C].  fp64 on the widened fp32 inputs.  For the sample (u, v) - a pixel centre is (u, v) integer:
 *     xd = (u - cx) / fx;  yd = (v - cy) / fy;  (x, y) = (xd, yd)
 *     20 times:  the terms above at (a, b) = (x, y);  s = den / num;  x = (xd - tx) * s;  y = (yd - ty) * s      (both from the old x, y)
 *     once more the terms at (x, y), rad = num / den, and (u', v') by the last two lines above
 *     the sample CONVERGED iff |u' - u| <= 1e-3 and |v' - v| <= 1e-3 and num > 0 and den > 0           (a NaN: not converged)
 *     rays[c][v][u] = ((float)x, (float)y) for a converged pixel centre, else (NaN, NaN)
 * Twenty steps is a definition, not a tuning result.  limit[c] = the largest r2 = fl(fl(xf * xf) + fl(yf * yf)), fp32 with
 * (xf, yf) = ((float)x, (float)y) - the forward model's own r2 of a point on that ray at Z = 1 - over the converged samples: the
 * H * W pixel centres and the image rectangle's boundary at half-pixel positions, (i - 0.5, -0.5) and (i - 0.5, H - 0.5) for
 * i = 0 .. W, (-0.5, j - 0.5) and (W - 0.5, j - 0.5) for j = 0 .. H; 0 when no sample converged.  complete[c] = 1 iff every pixel
 * centre has a ray.  A float maximum does not depend on its order.  Two launches: one thread per pixel centre writes the table;
 * one workgroup per camera then folds the table and the boundary samples (which it inverts itself) into limit and complete.
 * C == 0 or H * W == 0: SH_OK, nothing launched.  Null pointers, negative sizes: SH_ERR_INVALID_ARG; C > 65535 or H * W beyond 31
 * bits: SH_ERR_UNSUPPORTED.
 *
 * The _rays entry points: their namesakes' argument lists plus the calibration, and their namesakes' contracts with these changes.
 * rays_stride: the table images (coefficient rows, limits) per body - 1 (one camera) or V (a rig) - or 0: ONE table per camera,
 * [1] or [V], shared by all bodies; a rig's calibration does not depend on the body.  Camera (b, v) is image b * rays_stride + v.
 *   sh_depth_rays_count / _points, sh_depth_views_rays_count / _points (rays, rays_stride after stride): the point of a pixel is
 *       P = (fl(ra * z), fl(rb * z), z)   with (ra, rb) = rays[..][v][u]
 *     and the neighbours' points come from their own rays; intr is not read.  The tangent rule, the normal, "kept", the order,
 *     the padding and the rig transform are unchanged.  No kernel tests a ray for NaN: the caller masks the pixels without a ray
 *     (complete == 0).  All-zero coefficients agree with the pinhole entry points to rounding, not bit for bit: fl(ra * z) against
 *     fl(fl(fl(u - cx) * z) / fx).  The tile's rays are staged in LDS with the halo, next to z, in the same bank-free layout.
 *   sh_depth_views_rays_overlap (dist [..][8], limit [..], rays_stride after z_far): Q is projected by the forward model above.
 *   sh_free_space_views_rays_fwd / _bwd (rays, dist, limit, rays_stride after intr): the projection is the forward model, and in
 *     the c == 0 case (a, b) = rays[..][vq][uq], the ray of the nearest pixel that is not empty, replaces the pinhole ray; a NaN
 *     there: kind SH_FS_NONE, no term.  rx, ry, term and g keep their expressions: the term samples the nearest pixel and has
 *     no image gradient, so its backward pass needs no Jacobian of the lens.  cam may be NULL: one camera, V = 1, x in its frame
 *     (sh_free_space_fwd's case).  A view's LDS record grows by the 8 coefficients and the limit.
 * Limits: one model family - no fisheye or equidistant model -, one resolution per rig.
 */
SH_API int sh_camera_rays(const float* intr, const float* dist, int C, int H, int W, float* rays, float* limit, int32_t* complete,
                          sh_stream_t stream);
SH_API int sh_depth_rays_count(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, int B, int H, int W,
                               float z_near, float z_far, float max_step, int drop_isolated, int stride, const float* rays, int rays_stride,
                               int32_t* counts, void* workspace, size_t workspace_bytes, sh_stream_t stream);
SH_API int sh_depth_rays_points(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, int B, int H, int W,
                                float z_near, float z_far, float max_step, int drop_isolated, int stride, const float* rays, int rays_stride,
                                const int32_t* counts, int max_count, int M, const void* workspace, size_t workspace_bytes, float* points,
                                float* normals, int32_t* pixel, sh_stream_t stream);
SH_API int sh_depth_views_rays_count(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, const float* ext,
                                     int B, int V, int H, int W, float z_near, float z_far, float max_step, int drop_isolated, int stride,
                                     const float* rays, int rays_stride, int32_t* counts, void* workspace, size_t workspace_bytes,
                                     sh_stream_t stream);
SH_API int sh_depth_views_rays_points(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, const float* ext,
                                      int B, int V, int H, int W, float z_near, float z_far, float max_step, int drop_isolated, int stride,
                                      const float* rays, int rays_stride, const int32_t* counts, int max_count, int M, const void* workspace,
                                      size_t workspace_bytes, float* points, float* normals, int32_t* pixel, uint8_t* view,
                                      int32_t* view_first, sh_stream_t stream);
SH_API int sh_depth_views_rays_overlap(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask,
                                       const float* ext, int B, int V, int H, int W, float z_near, float z_far, const float* dist,
                                       const float* limit, int rays_stride, const float* points, const float* normals, const uint8_t* view,
                                       const int32_t* counts, int M, float tol, uint32_t* seen, uint8_t* keep, sh_stream_t stream);
SH_API int sh_free_space_views_rays_fwd(const float* x, int64_t x_sb, int rows, int n, const float* cam, const uint8_t* cls, const float* z,
                                        const int32_t* nearest, const float* intr, const float* rays, const float* dist, const float* limit,
                                        int rays_stride, int V, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin, int B,
                                        float* term, uint8_t* kind, float* loss, int32_t* counts, sh_stream_t stream);
SH_API int sh_free_space_views_rays_bwd(const float* x, int64_t x_sb, int rows, int n, const float* cam, const uint8_t* cls, const float* z,
                                        const int32_t* nearest, const float* intr, const float* rays, const float* dist, const float* limit,
                                        int rays_stride, int V, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin,
                                        const int32_t* counts, const float* gL, int B, float* g_x, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * GPU-resident dataset (autoencoder_dataset.py:26-58; main.py:209-237).  The reference loads and
 * normalises one .npy per sample in DataLoader worker processes; here the packed split is
 * normalised once on device and every batch is a row gather from the resident tensor.
 *
 * sh_dataset_normalize: raw contiguous [n][N][3] -> out contiguous [n][N+dummy_rows][3] (dummy rows
 * zero, :45-48), applying in the reference's order (:29-43) the steps selected by `flags`:
 *   ZEROMEAN  v -= mean_v(v)                      ZEROROOT  v -= sum_v j_root[v] * v   (J_regressor row 0)
 *   ONELENGTH v = v / (max_y - min_y) * 1.5       SMALL     v = v / 1.5
 *   GASS      v = (v - mean[N][3]) / stdv[N][3]   NORMAL    v = (v - center[n][3]) * scale[n][3]
 * then NaN -> 0.  Unused table pointers may be NULL.
 * sh_gather_meshes: out[j][:] = src[idx[j]][:] for j < b, rows of row_elems floats, idx int64 on
 * device (bit-exact copy; the caller guarantees 0 <= idx[j] < rows of src).
 */
enum sh_norm_flags {
    SH_NORM_ZEROMEAN = 1, SH_NORM_ZEROROOT = 2, SH_NORM_ONELENGTH = 4, SH_NORM_SMALL = 8, SH_NORM_GASS = 16, SH_NORM_NORMAL = 32
};
SH_API int sh_dataset_normalize(const float* raw, float* out, int n, int N, int dummy_rows, unsigned flags,
                         const float* j_root, const float* mean, const float* stdv, const float* center,
                         const float* scale, sh_stream_t stream);
SH_API int sh_gather_meshes(const float* src, int64_t row_elems, const int64_t* idx, int b, float* out, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Optimiser: torch.optim.Adam with coupled L2 weight decay (main.py:262; steps at
 * train_funcs.py:391-392, 509-510), multi-tensor.  For every tensor i < n_tensors, with t = steps[i][0] + 1:
 *   g' = g + weight_decay * p;  m = lerp(m, g', 1 - beta1);  v = beta2 * v + (1 - beta2) * g'^2;
 *   p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps);   then steps[i][0] += 1.
 * params / grads / exp_avg / exp_avg_sq / steps / numel are HOST arrays of length n_tensors holding
 * DEVICE pointers (steps[i]: one float, the number of updates applied so far) and element counts;
 * `lr` is a DEVICE scalar, so a captured launch follows learning-rate schedules and step counts
 * without re-capture.  An entry with numel[i] == 0 only advances steps[i] (its other pointers are not read): a parameter whose
 * update was applied by sh_linear_bwd_wgt_adam during backward.
 */
SH_API int sh_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, float* const* steps, const int64_t* numel, const float* lr,
                 double beta1, double beta2, double eps, double weight_decay, sh_stream_t stream);
/* steps[i][0] += 1 for i < n_tensors (HOST array of DEVICE pointers): the step counts of parameters whose update was applied by
 * sh_linear_bwd_wgt_adam during backward. */
SH_API int sh_adam_bump(int n_tensors, float* const* steps, sh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The small loss terms of the semantic loop as kernels.  x tensors are [B] meshes of rows of 3 floats,
 * batch stride x_bs floats (the dummy row may be present: faces / J never index it).  Deterministic (no atomics).
 *  - joint regression kps[b][j][:] = sum_v J[j][v] x[b][v][:] (train_funcs.py:131,161,230,296,336), J dense [K][N];
 *    sh_joint_l1_loss_fwd also returns loss[0] = mean |kps[:, keep] - target| (F.l1_loss, :231,:342; keep int32 [Kk],
 *    target [B][Kk][3]); _bwd OVERWRITES grad [B][N1][3] (gradient w.r.t. x; rows >= N get 0) from the saved kps.
 *  - part volume ratio (cal_volloss :56-71 averaged over the batch :323-330): parts as CSR over faces (pf_ptr [P+1], pf),
 *    vol [2][B][P] receives the signed volumes of (x_rec, x_gt); loss[0] = (1/P) sum_p mean_b | |vr/vg| - 1 |.
 *    _bwd: face_slot [F] = position of the face's part in the list or -1; vptr / vcorner as for the edge loss.
 *  - sh_zpart_reg (zpartreg :145-152): z [B][P][L], measure [B][M], part_idx / measure_idx int32 [n];
 *    loss[0] = mean | |z_p| / m - 1 | (relat) or | |z_p| - m |; with dz != NULL also writes gscale[0] * d loss / d z
 *    (loss may then be NULL). */
SH_API int sh_joint_regress(const float* x, int64_t x_bs, const float* J, int B, int N, int K, float* kps, sh_stream_t stream);
SH_API int sh_joint_l1_loss_fwd(const float* x, int64_t x_bs, const float* J, const int32_t* keep, const float* target, int B,
                                int N, int K, int Kk, float* kps, float* loss, sh_stream_t stream);
SH_API int sh_joint_l1_loss_bwd(const float* kps, const int32_t* keep, const float* target, const float* J, int B, int N1, int N,
                                int K, int Kk, const float* gscale, float* grad, sh_stream_t stream);
SH_API int sh_part_volume_loss_fwd(const float* x_rec, const float* x_gt, int64_t x_bs, const int32_t* faces,
                                   const int32_t* pf_ptr, const int32_t* pf, int B, int P, float* vol, float* loss,
                                   sh_stream_t stream);
SH_API int sh_part_volume_loss_bwd(const float* x_rec, int64_t x_bs, const int32_t* faces, const int32_t* face_slot,
                                   const int32_t* vptr, const int32_t* vcorner, const float* vol, int B, int P, int N1,
                                   const float* gscale, float* grad, sh_stream_t stream);
SH_API int sh_zpart_reg(const float* z, const float* measure, const int32_t* part_idx, const int32_t* measure_idx, int B, int P,
                        int L, int M, int n, int relat, float* loss, float* dz, const float* gscale, sh_stream_t stream);
/*  - joints <-> bones (utils_SH.py:26-84; inputs of the loop, no gradient).  sh_kps2skl: kps [B][J][3], bone k = joint i0[k] -
 *    (joint i1[k] + joint i2[k]) / 2 (i2 == i1 for two-joint bones), n = |bone|; mode 0: out [B][n_bones][4] = (bone / n, n),
 *    1: (bone, n), 2: [..][3] = bone (the pair loss's bone directions, :449-452), 3: [..][1] = n.  sh_skl2kps: skl
 *    [B][n_bones][4] (mode 0: direction * length; 1: first three) or [..][3] (mode 2); joints rebuilt in list order, joint
 *    tail[k] = joint head[k] - bone k with unassigned joints at the origin (n_joints <= 64), out [B][n_keep][3] = joints keep[].
 *    Operation for operation the arithmetic of the tensor-op forms (same bits).
 *  - sh_weighted_sum: out[0] = w0 t0 + w1 t1 + ... summed in sequence (terms: HOST array of n <= 16 DEVICE scalars, weights:
 *    HOST floats; a weight of exactly 1 leaves its term unscaled) when out != NULL; grads[i] = gscale[0] * w_i when grads !=
 *    NULL - the loop's `loss = loss + w * term` chain and its backward as one launch each. */
SH_API int sh_kps2skl(const float* kps, int B, int J, const int32_t* i0, const int32_t* i1, const int32_t* i2, int n_bones, int mode,
                      float* out, sh_stream_t stream);
SH_API int sh_skl2kps(const float* skl, int B, int n_bones, int mode, const int32_t* head, const int32_t* tail, int n_joints,
                      const int32_t* keep, int n_keep, float* out, sh_stream_t stream);
SH_API int sh_weighted_sum(int n, const float* const* terms, const float* weights, float* out, const float* gscale, float* grads,
                           sh_stream_t stream);

/* =============================================================================================
 * bf16 compute path (BASELINE.json configs[2]: "batch=512 bf16, DDP 8x"; the reference itself is fp32-only,
 * models.py:45).  Same operators as above with bf16 activations and bf16 working copies of the weights,
 * fp32 accumulation inside the kernels (v_mfma_f32_16x16x32_bf16), fp32 bias / activation arithmetic, and
 * fp32 master weights, gradients and Adam state outside them.  Tensors carry an explicit element type:
 */
enum sh_dtype { SH_DTYPE_F32 = 0, SH_DTYPE_BF16 = 1 };

/* Working copy of a SpiralConv weight: bf16, pre-ordered into the 1-KiB MFMA fragments the conv kernel keeps in
 * LDS (frag[k-step][16-channel tile][lane][8]; layout in csrc/sh_bf16.h), zero-padded.  `transpose` = 0 gives the
 * forward operand (Cg = Cin gathered channels, Nout = Cout), 1 the backward-data operand (Cg = Cout, Nout = Cin)
 * of the same fp32 master weight [Cout][S*Cin] (models.py:17).  sh_conv_wfrag_bytes(S, Cg, Nout) sizes the buffer
 * (16-byte aligned).  One launch converts all layers of a stack. */
SH_API size_t sh_conv_wfrag_bytes(int S, int Cg, int Nout);
SH_API int sh_conv_wfrag_prep_multi(int n_layers, const float* const* weight, void* const* wfrag, const int* S,
                                    const int* Cin, const int* Cout, const int* transpose, sh_stream_t stream);

/* sh_spiral_conv_fwd / sh_spiral_conv_bwd_data (models.py:40-51 and its autograd) in bf16.  Strides are in ELEMENTS
 * of the tensor's own type.  x / dpre: bf16 with 16 or a multiple of 32 channels, or fp32 with exactly 3 channels
 * (the xyz input of the first layer, the xyz gradient entering the last one); y / dx: bf16, or fp32 when it has
 * <= 16 channels (x_hat, dL/dx).  bias fp32; yprev bf16.  Other shapes: SH_ERR_UNSUPPORTED (use the fp32 entry
 * points, which take any shape). */
SH_API int sh_spiral_conv_fwd_bf16(const void* x, int x_dtype, int64_t x_sv, int64_t x_sb, const int32_t* table,
                                   const void* wfrag, const float* bias, void* y, int y_dtype, int64_t y_sv, int64_t y_sb,
                                   int B, int R, int S, int Cin, int Cout, int act, int zero_row, sh_stream_t stream);
SH_API int sh_spiral_conv_bwd_data_bf16(const void* dpre, int dp_dtype, int64_t dp_sv, int64_t dp_sb,
                                        const int32_t* table_t, const void* wfrag_t, void* dx, int dx_dtype,
                                        int64_t dx_sv, int64_t dx_sb, const void* yprev, int64_t yp_sv, int64_t yp_sb,
                                        int act_prev, int zero_row, int B, int n_in, int S, int Cin, int Cout,
                                        sh_stream_t stream);

/* Weight gradient of a 16 -> 3 channel layer (the decoder's last conv, models.py:146-153) in role-swapped form:
 *   dW[co][s][ci] = sum_{u,b} x[u,b,ci] * dpre_ext[table_t[u,s], b, co]
 * x is read once and the three-channel gradient is gathered through the TRANSPOSED table - the table and the extended
 * gradient buffer (rows of irregular vertices pre-summed behind the R real rows) that sh_spiral_conv_bwd_data[_bf16] takes,
 * so the caller runs the pre-sum launches first.  dpre_ext fp32 [rows][B][3], x [n_in][B][16] of the path's dtype, both
 * vertex-major and contiguous; needs R == n_in, B % 16 == 0 and S <= 10 (fp32 path: S <= 30, run as two or three launches over
 * shares of the positions) - sh_spiral_conv_bwd_wgt_thin_ok() tells.  Writes
 * partial slabs into `workspace` in the layout and count of sh_spiral_conv_bwd_wgt (path_dtype SH_DTYPE_F32) or
 * sh_spiral_conv_bwd_wgt_bf16 (SH_DTYPE_BF16): the matching ..._reduce_multi launch finishes dW and dbias.
 * dx != NULL: the same launch also writes the layer's backward-data (what sh_spiral_conv_bwd_data[_bf16] computes from the
 * same table and buffer): dx[u,b,:] = act_prev'(x[u,b,:]) * sum_s dpre_ext[table_t[u,s],b,:] . W[:, s, :], row zero_prev
 * forced to zero; dx [n_in (+ extra)][B][16] vertex-major of the path's dtype, weight = the fp32 master [3][S*16] (rounded to
 * bf16 in the kernel on the bf16 path, like the fragment copies); x is both the layer input and the activation output
 * whose derivative multiplies (act_prev = SH_ACT_IDENTITY: no factor).  dx_planes != NULL (fp32 path, with dx): the three-plane
 * image of dx's n_in rows (see the ..._p3 entry points) is written with them. */
SH_API int sh_spiral_conv_bwd_wgt_thin_ok(int B, int n_in, int S, int Cin, int Cout, int path_dtype);
SH_API int sh_spiral_conv_bwd_wgt_thin(const float* dpre_ext, int64_t dp_sv, int64_t dp_sb, const void* x, int x_dtype, int64_t x_sv,
                                int64_t x_sb, const int32_t* table_t, void* workspace, size_t workspace_bytes,
                                const float* weight, void* dx, int64_t dx_sv, int64_t dx_sb, void* dx_planes, int act_prev,
                                int zero_prev, int B, int R, int n_in, int S, int Cin, int Cout, int path_dtype, sh_stream_t stream);

/* sh_spiral_conv_bwd_wgt in bf16: x / dpre bf16 (channels % 8 == 0) or fp32 with exactly 3 channels; writes fp32 partial
 * slabs into `workspace` (>= sh_spiral_conv_bwd_wgt_workspace_bf16 bytes); sh_spiral_conv_bwd_wgt_reduce_multi_bf16 sums
 * the slabs of up to 16 layers into fp32 dW / dbias (same contract as the fp32 pair above). */
SH_API size_t sh_spiral_conv_bwd_wgt_workspace_bf16(int B, int R, int S, int Cin, int Cout);
SH_API int sh_spiral_conv_bwd_wgt_bf16(const void* dpre, int dp_dtype, int64_t dp_sv, int64_t dp_sb, const void* x, int x_dtype,
                                       int64_t x_sv, int64_t x_sb, const int32_t* table, void* workspace,
                                       size_t workspace_bytes, int B, int R, int S, int Cin, int Cout, sh_stream_t stream);
SH_API int sh_spiral_conv_bwd_wgt_reduce_multi_bf16(int n_layers, const void* const* workspaces, float* const* dW,
                                                    float* const* dbias, const int* B, const int* R, const int* S,
                                                    const int* Cin, const int* Cout, sh_stream_t stream);

/* The latent dense layers (models.py:85-86,130,144) in bf16: `weight_bf16` is a bf16 working copy [N][K] of the fp32
 * master weight (sh_cast_f32_to_bf16, or written by sh_adam_step_bf16 as it updates the master); x / dy / y / dx are bf16
 * or fp32 (the latent code and its gradient stay fp32); bias, dW, dbias fp32.  N and K must be multiples of 8, M is free.
 * workspace >= sh_linear_workspace_bf16(M, N, K) bytes, 16-byte aligned (split-reduction partials). */
SH_API size_t sh_linear_workspace_bf16(int M, int N, int K);
SH_API int sh_cast_f32_to_bf16(const float* src, void* dst, int64_t n, sh_stream_t stream);
SH_API int sh_linear_fwd_bf16(const void* x, int x_dtype, const void* weight_bf16, const float* bias, void* y, int y_dtype,
                              int M, int N, int K, void* workspace, size_t workspace_bytes, sh_stream_t stream);
SH_API int sh_linear_bwd_data_bf16(const void* dy, int dy_dtype, const void* weight_bf16, void* dx, int dx_dtype, int M, int N,
                                   int K, void* workspace, size_t workspace_bytes, sh_stream_t stream);
SH_API int sh_linear_bwd_wgt_bf16(const void* dy, int dy_dtype, const void* x, int x_dtype, float* dW, float* dbias, int M,
                                  int N, int K, sh_stream_t stream);

/* sh_spmm / sh_act_backward on bf16 tensors (channels % 8 == 0, 16-byte aligned rows; strides in bf16 elements; CSR values
 * fp32; arithmetic fp32, one rounding of the result). */
SH_API int sh_spmm_bf16(const int32_t* rowptr, const int32_t* col, const float* val, const void* x, int64_t x_sv, int64_t x_sb,
                        void* y, int64_t y_sv, int64_t y_sb, const void* yprev, int64_t yp_sv, int64_t yp_sb, int act_prev,
                        int zero_row, int B, int rows, int C, sh_stream_t stream);
SH_API int sh_act_backward_bf16(const void* dy, int64_t dy_sv, int64_t dy_sb, const void* y, int64_t y_sv, int64_t y_sb,
                                void* dpre, int64_t dp_sv, int64_t dp_sb, int B, int R, int C, int act, int zero_row,
                                sh_stream_t stream);

/* sh_adam_step that also rewrites, for every tensor with shadow_bf16[i] != NULL, a bf16 working copy of the updated fp32
 * parameter (same element order): the next forward pass reads the working copy without a separate conversion pass. */
SH_API int sh_adam_step_bf16(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                             float* const* exp_avg_sq, float* const* steps, void* const* shadow_bf16, const int64_t* numel,
                             const float* lr, double beta1, double beta2, double eps, double weight_decay, sh_stream_t stream);

/* sh_stack_forward / sh_stack_backward for the bf16 path.  Tensors between steps are bf16 vertex-major; x is bf16, or fp32
 * with 3 channels; the output of the last step has type out_dtype (fp32 only for <= 16 channels), g the same type; gin[0]
 * has type gx_dtype; dpre_last has the type of the last step's output.  wfrag[i] / wfrag_t[i]: per conv step, buffers of
 * sh_conv_wfrag_bytes(S, cin, cout) / (S, cout, cin) bytes which the call fills from the fp32 master `weights` (one
 * conversion launch per pass) - unless wfrag_ready != 0: then they already hold the converted CURRENT weights (the caller
 * ran sh_conv_wfrag_prep_multi itself, e.g. once for both stacks and both orientations of a training step) and no
 * conversion is launched.  workspace[i] >= sh_spiral_conv_bwd_wgt_workspace_bf16.  Everything else as above, dW[p] == NULL
 * included (no weight gradient for parameter p: no bf16 weight-gradient launch, no reduction job, no role-swapped 16 -> 3 kernel). */
SH_API int sh_stack_forward_bf16(int n_steps, const sh_stack_step* steps, const void* x, int x_dtype, int x_layout, int rows0,
                                 int c0, int B, const float* const* weights, const float* const* biases, void* const* wfrag,
                                 int wfrag_ready, void* const* outs, int out_dtype, int out_layout, sh_stream_t stream);
SH_API int sh_stack_backward_bf16(int n_steps, const sh_stack_step* steps, const void* x, int x_dtype, int x_layout, int rows0,
                                  int c0, int B, const void* const* acts, const void* g, int out_dtype, int out_layout,
                                  const float* const* weights, void* const* gin, int gx_dtype, void* dpre_last,
                                  void* const* wfrag_t, int wfrag_ready, void* const* workspace,
                                  const size_t* workspace_bytes, float* const* dW, float* const* dbias, int need_x_grad,
                                  sh_stream_t stream);

/* =============================================================================================
 * Three-plane form of the fp32 path's matrix products (round 4).  Same operators, same fp32 tensors at every interface
 * as the fp32 entry points above (models.py:34-53 and its autograd); what changes is where the exact bf16x3 operand
 * split of SH_MMA_SPLIT3 happens: the PRODUCER of an activation / gradient writes, beside the fp32 tensor, its three
 * bf16 planes v = h + m + l (exact) once, and the conv kernels gather the planes and only multiply (six - or with
 * SH_P3_NP=9 all nine - partial products on v_mfma_f32_16x16x32_bf16, fp32 accumulation).
 *
 * Plane image of a tensor [rows][B][C], B % 16 == 0, C == 16 or C % 32 == 0 (sh_p3_bytes(rows, B, C) bytes, 0 =
 * unsupported shape; 16-byte aligned): fragment-major - the B-operand order of the matrix instruction, so a wave's gather
 * is one contiguous 1-KiB access (layout in csrc/p3_conv.hip).  sh_to_p3 converts rows of an fp32 tensor (strides as
 * everywhere: element (r, b, c) at x + r*sv + b*sb + c); the conv entry points can also write the image of their output
 * (yp / dxp != NULL; then Cout resp. Cin must be 16 or a multiple of 32) next to - or instead of (y / dx == NULL) - the
 * fp32 tensor.  Weights: sh_conv_wfrag3_prep_multi = sh_conv_wfrag_prep_multi with three planes per fragment
 * (sh_conv_wfrag3_bytes).  sh_spiral_conv_p3_ok(B, S, Cg, Nout): 1 when the kernels take a layer with Cg gathered and
 * Nout produced channels (its three-plane weight must fit LDS); otherwise the caller keeps the exact kernels. */
SH_API size_t sh_p3_bytes(int rows, int B, int C);
SH_API int sh_to_p3(const float* x, int64_t x_sv, int64_t x_sb, void* planes, int B, int rows, int C, sh_stream_t stream);
SH_API size_t sh_conv_wfrag3_bytes(int S, int Cg, int Nout);
SH_API int sh_conv_wfrag3_prep_multi(int n_layers, const float* const* weight, void* const* wfrag3, const int* S, const int* Cin,
                                     const int* Cout, const int* transpose, sh_stream_t stream);
SH_API int sh_spiral_conv_p3_ok(int B, int S, int Cg, int Nout);
/* 0: not taken; 1: LDS-resident weight (backward-data also takes rows without an image: dpre_f32 below); 2: streamed weight */
SH_API int sh_spiral_conv_p3_kind(int B, int S, int Cg, int Nout);
/* Diagnostics (like sh_profile_*; selects nothing): the number of plane-conv kernel launches (conv_p3 / conv_p3s, forward and
 * backward-data) this process has issued so far.  A caller that asked for SH_MMA_PLANES3 can tell whether the plane kernels
 * really ran or the SPLIT3 kernels served the call (batch not a multiple of 16, shapes sh_spiral_conv_p3_ok() refuses):
 * tests/conftest.py reports the [planes3] instance of a test that never moved this counter as skipped, not passed. */
SH_API int64_t sh_p3_launch_count(void);
/* sh_spmm that also writes the plane image of the rows it produces (y_planes: image of row 0 of y; NULL = plain sh_spmm);
 * y == NULL with y_planes: the image alone (y_sv / y_sb still describe the vertex-major tensor the image belongs to) */
SH_API int sh_spmm_p3(const int32_t* rowptr, const int32_t* col, const float* val, const float* x, int64_t x_sv, int64_t x_sb,
                      float* y, int64_t y_sv, int64_t y_sb, void* y_planes, const float* yprev, int64_t yp_sv, int64_t yp_sb,
                      int act_prev, int zero_row, int B, int rows, int C, sh_stream_t stream);
/* sh_spiral_conv_fwd / sh_act_backward_tr that also write the plane image of what they store (y_planes / dpre_planes != NULL;
 * vertex-major result).  The conv writes it in its own epilogue where the kernel the dispatch picks has one, and issues
 * sh_to_p3 itself otherwise: the image is complete when the call returns either way. */
SH_API int sh_spiral_conv_fwd_img(const float* x, int64_t x_sv, int64_t x_sb, const int32_t* table, const float* weight,
                                  const float* bias, float* y, int64_t y_sv, int64_t y_sb, void* y_planes, int B, int R, int S, int Cin,
                                  int Cout, int act, int zero_row, int mma_mode, sh_stream_t stream);
SH_API int sh_act_backward_tr_img(const float* dy, int64_t dy_sv, int64_t dy_sb, const float* y, int64_t y_sv, int64_t y_sb, float* dpre,
                                  int64_t dp_sv, int64_t dp_sb, void* dpre_planes, int B, int R, int C, int act, int zero_row, int n_layers,
                                  const float* const* weight, float* const* weight_t, const int* S, const int* Cin, const int* Cout,
                                  sh_stream_t stream);
/* sh_spiral_conv_fwd with x given as its plane image xp ([n_in] rows).
 * Size limit of the gathered image (here and in sh_spiral_conv_bwd_data_p3): the kernels keep table entries pre-multiplied by
 * the image's row stride in 16-byte units in 32 bits, so the image must be smaller than 64 GiB (rows x B x C x 6 bytes); the
 * same holds for the fp32 tensor x of the streaming weight gradients (sh_spiral_conv_bwd_wgt*: rows x B x C x 4 bytes).  The
 * entry points do not know the gathered tensor's row count and cannot check it; sh_stack_forward / sh_stack_backward refuse
 * any tensor of 2^32 elements or more (SH_ERR_UNSUPPORTED), which is inside both limits. */
SH_API int sh_spiral_conv_fwd_p3(const void* xp, const int32_t* table, const void* wfrag3, const float* bias, float* y, int64_t y_sv,
                                 int64_t y_sb, void* yp, int B, int R, int S, int Cin, int Cout, int act, int zero_row,
                                 sh_stream_t stream);
/* sh_spiral_conv_bwd_data_z with dpre given as its plane image dprep (dpre_zero_row >= 0: the all-zero row the "no source"
 * entries point at - their products are skipped, bitwise the same result).  dpre_f32 != NULL: only rows < n_image_rows of dprep
 * are valid; the rows behind them (the pre-summed rows the transposed table refers to) are read from the fp32 tensor
 * (element strides dp_sv, dp_sb) and split by the kernel - their producers then need not write images.  yprev_planes (round 6;
 * may be NULL): the plane image of yprev ([n_in] rows x Cin channels) - the activation derivative is then evaluated from it
 * (h + m + l is the fp32 value, bit for bit) instead of from the fp32 tensor, which the caller need not keep cache-warm. */
SH_API int sh_spiral_conv_bwd_data_p3(const void* dprep, int dpre_zero_row, const float* dpre_f32, int64_t dp_sv, int64_t dp_sb,
                                      int n_image_rows, const int32_t* table_t, const void* wfrag3_t, float* dx, int64_t dx_sv,
                                      int64_t dx_sb, void* dxp, const float* yprev, int64_t yp_sv, int64_t yp_sb,
                                      const void* yprev_planes, int act_prev, int zero_row, int B, int n_in, int S, int Cin, int Cout,
                                      sh_stream_t stream);

/* sh_spiral_conv_bwd_data_p3 over RAGGED source lists (round 6; csrc/p3_conv.hip conv_p3r_kernel): dx[u] = act'(yprev[u]) x
 * sum_j dpre[rag_rows[u][j]] . W_{rag_pos[u][j]} over the entries with rag_pos >= 0 - no transposed table, no "no source" slots,
 * no pre-summed rows: the sums over several sources of one (row, position) are formed by the matrix pipe (linearity).  Every
 * source is a row of the image dprep.  sh_spiral_conv_p3_rag_ok: resident three-plane weight with at most four channel tiles per
 * workgroup, gathered channels (Cg = the layer's Cout) a multiple of 32, lists of at most 64 entries. */
SH_API int sh_spiral_conv_p3_rag_ok(int B, int S, int Cg, int Nout, int rag_L);
SH_API int sh_spiral_conv_bwd_data_p3_rag(const void* dprep, const int32_t* rag_rows, const int32_t* rag_pos, int rag_L, const void* wfrag3_t,
                                          float* dx, int64_t dx_sv, int64_t dx_sb, void* dxp, const float* yprev, int64_t yp_sv,
                                          int64_t yp_sb, const void* yprev_planes, int act_prev, int zero_row, int B, int n_in, int S,
                                          int Cin, int Cout, sh_stream_t stream);

/* Plane conv over GROUPED lists (csrc/p3_conv.hip conv_p3g_kernel, round 6): up to four output rows whose source lists overlap form a
 * group and share ONE list of the union of their sources - y[g_out[k][m]] = sum over the entries j of group k that member m reads
 * (byte m of g_pos[k][j] != 0xFF) of x[g_rows[k][j]] . W_{that byte} - so every row of the union is gathered once where the
 * one-row kernels (sh_spiral_conv_fwd_p3 through the table, sh_spiral_conv_bwd_data_p3_rag through ragged lists) gather it once
 * per member; matrix work and results' arithmetic are theirs (the order of a row's partial sums follows the group's list).
 * backward == 0: the forward pass (x = image of the layer input, wfrag3 = forward fragments, bias, activation `act`, masked
 * zero_row; Cg = the layer's Cin, Nout = its Cout, R = its output rows); backward == 1: backward-data (x = image of the
 * pre-activation gradient, wfrag3 = transposed fragments, the derivative of activation `act` at yprev / yprev_planes - the fp32
 * tensor or the image of the layer input - or neither; Cg = the layer's Cout, Nout = its Cin, R = its input rows).  y and / or yp
 * (the image of the result) are written.  .._grp_ok: resident three-plane weight with at most four channel tiles per workgroup,
 * Cg a multiple of 32, or 16 with at most two channel tiles (a k-step then spans two list entries), lists of at most 64 entries; .._grp_members: how many members per group the kernel of this shape takes (4 or 2;
 * 0 = shape not taken) - g_out always has four slots per group. */
SH_API int sh_spiral_conv_p3_grp_ok(int B, int S, int Cg, int Nout, int g_L);
SH_API int sh_spiral_conv_p3_grp_members(int B, int S, int Cg, int Nout);
/* 1 when the launch has enough groups x batch groups to fill the chip with its coarser work items (the sequencers' rule for taking
 * the grouped form: 12 work items per CU). */
SH_API int sh_spiral_conv_p3_grp_pays(int B, int n_groups);
SH_API int sh_spiral_conv_p3_grp(const void* xp, const int32_t* g_rows, const uint32_t* g_pos, const int32_t* g_out, int n_groups, int g_L,
                                 const void* wfrag3, const float* bias, float* y, int64_t y_sv, int64_t y_sb, void* yp, const float* yprev,
                                 int64_t yp_sv, int64_t yp_sb, const void* yprev_planes, int act, int zero_row, int backward, int B, int R,
                                 int S, int Cg, int Nout, sh_stream_t stream);

/* The same over bf16 tensors (csrc/bf16_conv.hip conv_bf16r_kernel; the ragged sibling of sh_spiral_conv_bwd_data_bf16): dpre and dx
 * bf16 (element strides), wfrag_t the transposed bf16 fragments of sh_conv_wfrag_prep_multi, yprev bf16 or NULL.  The sums over
 * several sources of one (row, position) are formed in fp32 by the matrix pipe, where the dense form reads pre-summed rows that
 * were rounded to bf16 once more.  .._rag_ok: gathered channels (the layer's Cout) a multiple of 32, output channels a multiple
 * of 4, lists of at most 64 entries, a weight slice that fits LDS. */
SH_API int sh_spiral_conv_bf16_rag_ok(int B, int S, int Cg, int Nout, int rag_L);
SH_API int sh_spiral_conv_bwd_data_bf16_rag(const void* dpre, int64_t dp_sv, int64_t dp_sb, const int32_t* rag_rows, const int32_t* rag_pos,
                                            int rag_L, const void* wfrag_t, void* dx, int64_t dx_sv, int64_t dx_sb, const void* yprev,
                                            int64_t yp_sv, int64_t yp_sb, int act_prev, int zero_row, int B, int n_in, int S, int Cin,
                                            int Cout, sh_stream_t stream);

/* Weight gradient of a spiral conv in the three-plane form (csrc/wgrad_p3.hip, round 6; autograd of reference models.py:45,
 * dW = dpre^T . gather(x)): both operands given as their plane images - x_planes = image of the layer's input ([n_in] rows,
 * what its forward plane conv gathered), dpre_planes = image of the pre-activation gradient (rows [0, R) are read) - six
 * bf16 partial products per fp32 product, fp32 accumulation, the arithmetic of sh_spiral_conv_fwd_p3.  Writes partial slabs
 * (dW and dbias) into workspace, in the layout and for the deferred reduction of sh_spiral_conv_bwd_wgt(dW == NULL):
 * sh_spiral_conv_bwd_wgt_reduce_multi_kinds (kind 2).  .._p3_ok: 1 when the kernel takes the shape (batch % 16 == 0, Cin 16 or a
 * multiple of 32, Cout a multiple of 32); otherwise the caller keeps sh_spiral_conv_bwd_wgt.  dpre_zero_row: a row of dpre that
 * is all zero (the layer's dummy row), or -1 - needed only when R * (B / 16) is odd: the kernel sums pairs of 16-row units and
 * completes an odd count with that row's (SH_ERR_UNSUPPORTED without one). */
SH_API int sh_spiral_conv_bwd_wgt_p3_ok(int B, int R, int S, int Cin, int Cout);
SH_API size_t sh_spiral_conv_bwd_wgt_p3_workspace(int B, int R, int S, int Cin, int Cout);
SH_API int sh_spiral_conv_bwd_wgt_p3(const void* dpre_planes, int dpre_zero_row, const void* x_planes, const int32_t* table, void* workspace,
                                     size_t workspace_bytes, int B, int R, int S, int Cin, int Cout, sh_stream_t stream);
/* The same launch also carrying a pre-sum job, as sh_spiral_conv_bwd_wgt_presum does for the fp32 kernels: sum_out[r] = sum_e
 * sum_val[e] * dpre[sum_col[e]] for r < sum_rows over the FP32 gradient rows dpre (element strides dp_sv, dp_sb; sum_out has the
 * same strides; sum_out_planes != NULL: also the image of those rows) - sh_spmm's sums bit for bit, run by tail workgroups of
 * the launch (or, for rows that do not take 16-byte accesses, by sh_spmm_p3 in front of it).  sum_rows == 0: no job. */
SH_API int sh_spiral_conv_bwd_wgt_p3_presum(const void* dpre_planes, int dpre_zero_row, const void* x_planes, const int32_t* table,
                                            void* workspace, size_t workspace_bytes, const float* dpre, int64_t dp_sv, int64_t dp_sb,
                                            const int32_t* sum_rowptr, const int32_t* sum_col, const float* sum_val, float* sum_out,
                                            void* sum_out_planes, int sum_rows, int B, int R, int S, int Cin, int Cout,
                                            sh_stream_t stream);
/* sh_spiral_conv_bwd_wgt_reduce_multi over layers whose slabs were written under different plans: kinds[i] = 0 the fp32 plan
 * (sh_spiral_conv_bwd_wgt*, the thin-layer kernel), 1 the bf16 plan, 2 the three-plane plan (sh_spiral_conv_bwd_wgt_p3*). */
SH_API int sh_spiral_conv_bwd_wgt_reduce_multi_kinds(int n_layers, const void* const* workspaces, float* const* dW, float* const* dbias,
                                                     const int* B, const int* R, const int* S, const int* Cin, const int* Cout,
                                                     const int* kinds, sh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SH_KERNELS_H */
