// Torch bindings + launchers for the gfx950 SAE kernels (sae_kernels.hip).
// Built in-tree as sparse_coding_amd/ops/_sae_hip.so by ops/build.py.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include "sae_kernels.hip"

static inline void check_in(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
}
#define CHECK_IN(t) check_in(t, #t)

// optional fp32 tensor -> checked pointer, nullptr when absent
static inline float* opt_ptr(const c10::optional<torch::Tensor>& t, const char* name) {
  if (!t.has_value()) return nullptr;
  check_in(*t, name);
  return t->data_ptr<float>();
}
#define OPT_PTR(t) opt_ptr(t, #t)

static inline int* int32_ptr(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == torch::kInt32,
              name, " must be int32 GPU");
  return t.data_ptr<int>();
}

static inline hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// output-tile width LAUNCH_TILE_BN takes for a requested bn
static inline int tile_bn(int64_t bn) { return bn == 256 ? 256 : BN; }

// batch stride of x between models: 0 for a shared [B, d], B*d for [M, B, d]
static inline long x_model_stride(const torch::Tensor& x, int M) {
  if (x.dim() != 3) return 0;
  TORCH_CHECK(x.size(0) == M, "per-model x must be [M,B,d]");
  return (long)x.size(1) * x.size(2);
}

// Tile dispatch for the GEMM launchers, stated once.  The kernels are
// instantiated as <TBK, MINW, TBN, ALIGNED>: TBK 16 and 32 are the two depths
// of the 128x128 tile, <16, 4, 256> is the 128x256 tile.  LAUNCH_TILE picks by
// tile depth alone (kernels without a 256-wide variant); LAUNCH_TILE_BN takes
// the 256-wide one when bn == 256.  Each launcher states its grid and its
// argument list once.
//
// Every variant exists twice.  The guarded kernels take any shape.  The
// ALIGNED ones drop every row, column and K-tail guard, and are launched when
// the TileShape says that no guard could fire: rows % 128 == 0, cols % TBN ==
// 0, K % TBK == 0, the float4-staged operands 16-byte aligned with leading
// dimensions that are multiples of 4.  `mw16` is the aligned TBK=16 kernel's
// minimum waves per SIMD: 8 (four workgroups per CU) where it compiles to
// <= 64 VGPRs without scratch, else the guarded kernel's 6.
struct TileShape {
  long rows, cols, K;  // of the GEMM: output rows and columns, contraction
  bool operands_ok;    // base pointers and leading dimensions
  bool aligned(int tbn, int tbk) const {
    return operands_ok && rows % BM == 0 && cols % tbn == 0 && K % tbk == 0;
  }
};

static bool g_aligned_tiles = true;
void set_aligned_tiles(bool on) { g_aligned_tiles = on; }
bool aligned_tiles() { return g_aligned_tiles; }

// operands of one launch: a and b are staged with float4 loads, ld_out is the
// leading dimension of the epilogue's row-major operands (its per-lane byte
// offset, at most 4 * (127 * ld_out + 255), is kept in 32 bits)
static inline TileShape tile_shape(long rows, long cols, long K,
                                   const void* a, long lda, const void* b, long ldb,
                                   long ld_out) {
  auto ok = [](const void* p, long ld) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % 4 == 0;
  };
  return {rows, cols, K,
          g_aligned_tiles && ok(a, lda) && ok(b, ldb) && ld_out < (1L << 23)};
}

#define LAUNCH_AS(kern, grid, ...) \
  hipLaunchKernelGGL(kern, grid, dim3(NTHREADS), 0, cur_stream(), __VA_ARGS__)
#define LAUNCH_VARIANT(kern, tbk, mw, mw_aligned, tbn, shape, grid, ...)         \
  do {                                                                            \
    if ((shape).aligned(tbn, tbk))                                                \
      LAUNCH_AS((kern<tbk, mw_aligned, tbn, true>), grid, __VA_ARGS__);           \
    else                                                                          \
      LAUNCH_AS((kern<tbk, mw, tbn, false>), grid, __VA_ARGS__);                  \
  } while (0)
#define LAUNCH_TILE(kern, mw16, shape, bk, grid, ...)                             \
  do {                                                                            \
    if ((bk) == 16) LAUNCH_VARIANT(kern, 16, 6, mw16, BN, shape, grid, __VA_ARGS__); \
    else LAUNCH_VARIANT(kern, 32, 4, 4, BN, shape, grid, __VA_ARGS__);            \
  } while (0)
#define LAUNCH_TILE_BN(kern, mw16, shape, bn, bk, grid, ...)                      \
  do {                                                                            \
    if ((bn) == 256) LAUNCH_VARIANT(kern, 16, 4, 4, 256, shape, grid, __VA_ARGS__); \
    else LAUNCH_TILE(kern, mw16, shape, bk, grid, __VA_ARGS__);                   \
  } while (0)
// the pre-transposed pair has no aligned variants
#define LAUNCH_TILE_GUARDED(kern, bk, grid, ...)                  \
  do {                                                            \
    if ((bk) == 16) LAUNCH_AS((kern<16, 6>), grid, __VA_ARGS__);  \
    else LAUNCH_AS((kern<32, 4>), grid, __VA_ARGS__);             \
  } while (0)

void row_norms(torch::Tensor W, torch::Tensor norms, torch::Tensor inv_norms, double eps) {
  CHECK_IN(W); CHECK_IN(norms); CHECK_IN(inv_norms);
  long rows = W.numel() / W.size(-1);
  int d = W.size(-1);
  dim3 grid(cdiv(rows, NTHREADS / WAVE));
  hipLaunchKernelGGL(k_row_norms, grid, dim3(NTHREADS), 0, cur_stream(),
                     W.data_ptr<float>(), norms.data_ptr<float>(),
                     inv_norms.data_ptr<float>(), (int)rows, d, (float)eps);
}

void enc_fwd(torch::Tensor x, torch::Tensor Wenc, torch::Tensor bias,
             c10::optional<torch::Tensor> inv_norms, torch::Tensor c_out,
             torch::Tensor loss_parts, torch::Tensor fired, int64_t mode,
             int64_t bk, bool prio,
             int64_t bn,
             c10::optional<torch::Tensor> act_scale,
             c10::optional<torch::Tensor> act_gain,
             c10::optional<torch::Tensor> u_out,
             c10::optional<torch::Tensor> dict_sizes,
             c10::optional<torch::Tensor> y_in,
             c10::optional<torch::Tensor> x_prev,
             c10::optional<torch::Tensor> x_out,
             c10::optional<torch::Tensor> mom) {
  CHECK_IN(x); CHECK_IN(Wenc); CHECK_IN(bias); CHECK_IN(c_out);
  CHECK_IN(loss_parts); CHECK_IN(fired);
  int M = Wenc.size(0), n = Wenc.size(1), d = Wenc.size(2);
  const long x_mstride = x_model_stride(x, M);
  int B = x.size(x.dim() - 2);
  TORCH_CHECK(d % 4 == 0 && n % 4 == 0, "d and n must be multiples of 4 (float4 staging)");
  // which epilogue reads which optional operand; the others may be absent
  if (mode == ENC_GATE)
    TORCH_CHECK(act_scale && act_gain && u_out, "mode 2 needs act_scale/act_gain/u_out");
  if (mode == ENC_LISTA_FWD || mode == ENC_LISTA_BWD) TORCH_CHECK(y_in, "modes 4/5 need y_in");
  if (mode == ENC_LISTA_FWD)
    TORCH_CHECK(x_prev && x_out && mom && act_scale && u_out,
                "mode 4 needs x_prev/x_out/mom/act_scale(theta)/u_out");
  const int* ds_p = dict_sizes ? int32_ptr(*dict_sizes, "dict_sizes") : nullptr;
  dim3 grid(cdiv(n, tile_bn(bn)), cdiv(B, BM), M);
  const TileShape shape = tile_shape(B, n, d, x.data_ptr<float>(), d, Wenc.data_ptr<float>(), d, n);
  LAUNCH_TILE_BN(k_enc_fwd_t, 8, shape, bn, bk, grid,
                 x.data_ptr<float>(), Wenc.data_ptr<float>(),
                 bias.data_ptr<float>(), OPT_PTR(inv_norms), c_out.data_ptr<float>(),
                 loss_parts.data_ptr<float>(), fired.data_ptr<float>(),
                 B, d, n, (int)mode, prio ? 1 : 0, OPT_PTR(act_scale), OPT_PTR(act_gain),
                 OPT_PTR(u_out), ds_p, x_mstride,
                 OPT_PTR(y_in), OPT_PTR(x_prev), OPT_PTR(x_out), OPT_PTR(mom));
}

void dec_fwd(torch::Tensor c, torch::Tensor Wdec, torch::Tensor inv_norms,
             torch::Tensor x, torch::Tensor r_out, torch::Tensor loss_parts,
             int64_t bk, bool prio, int64_t bn) {
  CHECK_IN(c); CHECK_IN(Wdec); CHECK_IN(inv_norms); CHECK_IN(x);
  CHECK_IN(r_out); CHECK_IN(loss_parts);
  int M = Wdec.size(0), n = Wdec.size(1), d = Wdec.size(2);
  const long x_mstride = x_model_stride(x, M);
  int B = x.size(x.dim() - 2);
  dim3 grid(cdiv(d, tile_bn(bn)), cdiv(B, BM), M);
  const TileShape shape = tile_shape(B, d, n, c.data_ptr<float>(), n, Wdec.data_ptr<float>(), d, d);
  // the aligned TBK=16 kernel needs scratch at 8 waves/SIMD: it keeps 6
  LAUNCH_TILE_BN(k_dec_fwd_t, 6, shape, bn, bk, grid,
                 c.data_ptr<float>(), Wdec.data_ptr<float>(),
                 inv_norms.data_ptr<float>(), x.data_ptr<float>(),
                 r_out.data_ptr<float>(), loss_parts.data_ptr<float>(),
                 B, d, n, prio ? 1 : 0, x_mstride);
}

void gc(torch::Tensor r, torch::Tensor Wdec, torch::Tensor inv_norms,
        torch::Tensor c, torch::Tensor l1_alpha, torch::Tensor gpre,
        torch::Tensor g_bias, int64_t bk, bool prio, int64_t gc_mode, int64_t bn,
        bool accumulate) {
  CHECK_IN(r); CHECK_IN(Wdec); CHECK_IN(inv_norms); CHECK_IN(c);
  CHECK_IN(l1_alpha); CHECK_IN(gpre); CHECK_IN(g_bias);
  int M = Wdec.size(0), n = Wdec.size(1), d = Wdec.size(2);
  int B = r.size(1);
  dim3 grid(cdiv(n, tile_bn(bn)), cdiv(B, BM), M);
  // GC_RELU: the kernel stores one column sum per 32-row group; they are
  // added into g_bias in a fixed order below (reproducible bias gradient);
  // accumulate=false overwrites g_bias, so the caller need not zero it
  const int nrg = cdiv(B, 32);
  torch::Tensor part;
  float* part_p = nullptr;
  if (gc_mode == GC_RELU) {
    TORCH_CHECK(g_bias.numel() == (long)M * n, "g_bias must be [M, n]");
    part = torch::empty({M, nrg, n}, r.options());
    part_p = part.data_ptr<float>();
  }
  const TileShape shape = tile_shape(B, n, d, r.data_ptr<float>(), d, Wdec.data_ptr<float>(), d, n);
  LAUNCH_TILE_BN(k_gc_t, 8, shape, bn, bk, grid,
                 r.data_ptr<float>(), Wdec.data_ptr<float>(),
                 inv_norms.data_ptr<float>(), c.data_ptr<float>(),
                 l1_alpha.data_ptr<float>(), gpre.data_ptr<float>(),
                 part_p, B, d, n, prio ? 1 : 0, (int)gc_mode);
  if (gc_mode == GC_RELU) {
    long total = (long)M * n;
    hipLaunchKernelGGL(k_colsum_groups, dim3(cdiv(total, WAVE)), dim3(256), 0, cur_stream(),
                       part_p, g_bias.data_ptr<float>(), nrg, n, total, accumulate ? 1 : 0);
  }
}

void gc_thresh(torch::Tensor r, torch::Tensor Wdec, torch::Tensor inv_norms,
               torch::Tensor c, torch::Tensor u, torch::Tensor act_scale,
               torch::Tensor l1_alpha, torch::Tensor gpre,
               torch::Tensor g_gain, torch::Tensor g_scale,
               int64_t bk, bool prio) {
  CHECK_IN(r); CHECK_IN(Wdec); CHECK_IN(inv_norms); CHECK_IN(c); CHECK_IN(u);
  CHECK_IN(act_scale); CHECK_IN(l1_alpha); CHECK_IN(gpre);
  CHECK_IN(g_gain); CHECK_IN(g_scale);
  int M = Wdec.size(0), n = Wdec.size(1), d = Wdec.size(2);
  int B = r.size(1);
  dim3 grid(cdiv(n, BN), cdiv(B, BM), M);
  const TileShape shape = tile_shape(B, n, d, r.data_ptr<float>(), d, Wdec.data_ptr<float>(), d, n);
  LAUNCH_TILE(k_gc_thresh_t, 8, shape, bk, grid,
              r.data_ptr<float>(), Wdec.data_ptr<float>(),
              inv_norms.data_ptr<float>(), c.data_ptr<float>(),
              u.data_ptr<float>(), act_scale.data_ptr<float>(),
              l1_alpha.data_ptr<float>(), gpre.data_ptr<float>(),
              g_gain.data_ptr<float>(), g_scale.data_ptr<float>(),
              B, d, n, prio ? 1 : 0);
}

// gw[m] = beta * gw[m] + alpha * P[m]^T @ Q[m]; Q may be rank-shared [B, d]
void grad_w(torch::Tensor P, torch::Tensor Q, torch::Tensor gw,
            double alpha, double beta, int64_t bk, bool prio, int64_t bn) {
  CHECK_IN(P); CHECK_IN(Q); CHECK_IN(gw);
  int M = gw.size(0), n = gw.size(1), d = gw.size(2);
  int B;
  long p_stride, q_stride;
  TORCH_CHECK(P.dim() == 3, "P must be [M, B, n]");
  B = P.size(1);
  p_stride = (long)B * n;
  if (Q.dim() == 3) {
    q_stride = (long)B * d;
  } else {
    q_stride = 0;  // shared across models
  }
  dim3 grid(cdiv(d, tile_bn(bn)), cdiv(n, BM), M);
  const TileShape shape = tile_shape(n, d, B, P.data_ptr<float>(), n, Q.data_ptr<float>(), d, d);
  LAUNCH_TILE_BN(k_grad_w_t, 8, shape, bn, bk, grid,
                 P.data_ptr<float>(), p_stride, Q.data_ptr<float>(),
                 q_stride, gw.data_ptr<float>(), (float)alpha,
                 (float)beta, B, n, d, prio ? 1 : 0);
}

void project_adam(torch::Tensor W, torch::Tensor gw, torch::Tensor norms,
                  torch::Tensor mu, torch::Tensor nu, torch::Tensor step_no,
                  long n_per_model, double lr, double b1, double b2,
                  double eps_adam, double eps_norm, bool project,
                  c10::optional<torch::Tensor> w_used, bool clamp_mask,
                  c10::optional<torch::Tensor> lr_mult) {
  CHECK_IN(W); CHECK_IN(gw); CHECK_IN(norms); CHECK_IN(mu); CHECK_IN(nu);
  CHECK_IN(step_no);
  const float* wu = OPT_PTR(w_used);
  long rows = W.numel() / W.size(-1);
  const float* lrm = nullptr;
  if (lr_mult.has_value()) {
    CHECK_IN(lr_mult.value());
    TORCH_CHECK(lr_mult->numel() == rows, "lr_mult must have one entry per row");
    lrm = lr_mult->data_ptr<float>();
  }
  int d = W.size(-1);
  dim3 grid(cdiv(rows, NTHREADS / WAVE));
  hipLaunchKernelGGL(k_project_adam, grid, dim3(NTHREADS), 0, cur_stream(),
                     W.data_ptr<float>(), gw.data_ptr<float>(),
                     norms.data_ptr<float>(), mu.data_ptr<float>(),
                     nu.data_ptr<float>(), step_no.data_ptr<float>(),
                     (int)rows, (int)n_per_model, d, (float)lr, (float)b1,
                     (float)b2, (float)eps_adam, (float)eps_norm,
                     project ? 1 : 0, wu, clamp_mask ? 1 : 0, lrm);
}

void bias_adam(torch::Tensor bias, torch::Tensor g_bias, torch::Tensor decay,
               torch::Tensor mu, torch::Tensor nu, torch::Tensor step_no,
               double lr, double b1, double b2, double eps_adam,
               c10::optional<torch::Tensor> lr_mult) {
  CHECK_IN(bias); CHECK_IN(g_bias); CHECK_IN(decay); CHECK_IN(mu);
  CHECK_IN(nu); CHECK_IN(step_no);
  int M = bias.size(0), n = bias.size(1);
  const float* lrm = nullptr;
  if (lr_mult.has_value()) {
    CHECK_IN(lr_mult.value());
    TORCH_CHECK(lr_mult->numel() == (long)M * n, "lr_mult must match bias shape");
    lrm = lr_mult->data_ptr<float>();
  }
  hipLaunchKernelGGL(k_bias_adam, dim3(M), dim3(NTHREADS), 0, cur_stream(),
                     bias.data_ptr<float>(), g_bias.data_ptr<float>(),
                     decay.data_ptr<float>(), mu.data_ptr<float>(),
                     nu.data_ptr<float>(), step_no.data_ptr<float>(), n,
                     (float)lr, (float)b1, (float)b2, (float)eps_adam, lrm);
}

void colsum(torch::Tensor X, torch::Tensor out, double alpha, bool absval) {
  CHECK_IN(X); CHECK_IN(out);
  TORCH_CHECK(X.dim() == 3, "colsum wants [M, B, n]");
  int M = X.size(0), B = X.size(1), n = X.size(2);
  TORCH_CHECK(out.numel() == (long)M * n, "out must be [M, n]");
  int nsplit = std::min(std::max(B / 256, 1), 16);
  hipMemsetAsync(out.data_ptr<float>(), 0, (size_t)M * n * sizeof(float),
                 cur_stream());
  dim3 grid(cdiv(n, 256), M, nsplit);
  hipLaunchKernelGGL(k_colsum, grid, dim3(256), 0, cur_stream(),
                     X.data_ptr<float>(), out.data_ptr<float>(), B, n,
                     (float)alpha, absval ? 1 : 0);
}

void transpose_scale(torch::Tensor src, torch::Tensor dst,
                     c10::optional<torch::Tensor> scale) {
  CHECK_IN(src); CHECK_IN(dst);
  int R, C, M;
  long src_ms = 0, dst_ms = 0, scale_ms = 0;
  if (src.dim() == 3) {
    M = src.size(0); R = src.size(1); C = src.size(2);
    src_ms = (long)R * C; dst_ms = (long)R * C;
  } else {
    M = 1; R = src.size(0); C = src.size(1);
  }
  const float* sc = nullptr;
  if (scale.has_value()) {
    CHECK_IN(scale.value());
    sc = scale->data_ptr<float>();
    scale_ms = (src.dim() == 3) ? R : 0;
  }
  dim3 grid(cdiv(C, 64), cdiv(R, 64), M);
  hipLaunchKernelGGL(k_transpose_scale, grid, dim3(256), 0, cur_stream(),
                     src.data_ptr<float>(), dst.data_ptr<float>(), sc,
                     R, C, src_ms, dst_ms, scale_ms);
}

void enc_fwd2(torch::Tensor xT, torch::Tensor WT, torch::Tensor bias,
              torch::Tensor c_out, torch::Tensor loss_parts,
              torch::Tensor fired, int64_t mode, int64_t bk, bool prio,
              c10::optional<torch::Tensor> dict_sizes) {
  CHECK_IN(xT); CHECK_IN(WT); CHECK_IN(bias); CHECK_IN(c_out);
  CHECK_IN(loss_parts); CHECK_IN(fired);
  int M = WT.size(0), d = WT.size(1), n = WT.size(2);
  int B = xT.size(1);
  TORCH_CHECK(B % 4 == 0 && n % 4 == 0, "B and n must be multiples of 4");
  const int* ds_p = dict_sizes ? int32_ptr(*dict_sizes, "dict_sizes") : nullptr;
  dim3 grid(cdiv(n, BN), cdiv(B, BM), M);
  LAUNCH_TILE_GUARDED(k_enc_fwd2_t, bk, grid,
              xT.data_ptr<float>(), WT.data_ptr<float>(),
              bias.data_ptr<float>(), c_out.data_ptr<float>(),
              loss_parts.data_ptr<float>(), fired.data_ptr<float>(),
              B, d, n, (int)mode, prio ? 1 : 0, ds_p);
}

void gc2(torch::Tensor rT, torch::Tensor WT, torch::Tensor c,
         torch::Tensor l1_alpha, torch::Tensor gpre, torch::Tensor g_bias,
         int64_t bk, bool prio, int64_t gc_mode) {
  CHECK_IN(rT); CHECK_IN(WT); CHECK_IN(c); CHECK_IN(l1_alpha);
  CHECK_IN(gpre); CHECK_IN(g_bias);
  int M = WT.size(0), d = WT.size(1), n = WT.size(2);
  int B = rT.size(2);
  dim3 grid(cdiv(n, BN), cdiv(B, BM), M);
  LAUNCH_TILE_GUARDED(k_gc2_t, bk, grid,
              rT.data_ptr<float>(), WT.data_ptr<float>(),
              c.data_ptr<float>(), l1_alpha.data_ptr<float>(),
              gpre.data_ptr<float>(), g_bias.data_ptr<float>(),
              B, d, n, prio ? 1 : 0, (int)gc_mode);
}

void topk_select(torch::Tensor scores, torch::Tensor c_out, torch::Tensor fired,
                 torch::Tensor ks) {
  CHECK_IN(scores); CHECK_IN(c_out); CHECK_IN(fired);
  int M = scores.size(0), B = scores.size(1), n = scores.size(2);
  dim3 grid(B, 1, M);
  hipLaunchKernelGGL(k_topk_select, grid, dim3(TOPK_T), 0, cur_stream(),
                     scores.data_ptr<float>(), c_out.data_ptr<float>(),
                     fired.data_ptr<float>(), int32_ptr(ks, "ks"), B, n);
}

// int32 elements of workspace batch_topk_select needs for M models
int64_t batch_topk_workspace_size(int64_t M) { return M * (int64_t)BTK_WORK; }

// Batch-level top-k: a zeroing of the workspace, three histogram passes and
// one write pass, all on the current stream (capturable; no host read).  K =
// min(ks[m] * B, B * n) is computed on the device.
void batch_topk_select(torch::Tensor scores, torch::Tensor c_out, torch::Tensor fired,
                       torch::Tensor ks, torch::Tensor thr_out, torch::Tensor work,
                       c10::optional<torch::Tensor> threshold,
                       c10::optional<torch::Tensor> threshold_n,
                       c10::optional<torch::Tensor> threshold_lr) {
  CHECK_IN(scores); CHECK_IN(c_out); CHECK_IN(fired); CHECK_IN(thr_out);
  TORCH_CHECK(scores.dim() == 3, "scores must be [M,B,n]");
  TORCH_CHECK(c_out.sizes() == scores.sizes(), "c_out must have the shape of scores");
  const long M = scores.size(0), B = scores.size(1), n = scores.size(2);
  TORCH_CHECK(B * n < (1L << 31), "batch_topk_select: B*n per model must be below 2^31");
  TORCH_CHECK(M <= 65535, "batch_topk_select: at most 65535 models");
  TORCH_CHECK(fired.numel() == M * n, "fired must be [M,n]");
  TORCH_CHECK(ks.numel() == M && thr_out.numel() == M, "ks and thr_out must be [M]");
  TORCH_CHECK(work.numel() >= batch_topk_workspace_size(M),
              "work needs batch_topk_workspace_size(M) int32 elements");
  const int* ks_p = int32_ptr(ks, "ks");
  unsigned* work_p = reinterpret_cast<unsigned*>(int32_ptr(work, "work"));
  const bool has_thr = threshold.has_value();
  TORCH_CHECK(threshold_n.has_value() == has_thr && threshold_lr.has_value() == has_thr,
              "threshold, threshold_n and threshold_lr go together");
  float* th_p = nullptr; int* thn_p = nullptr; const float* thlr_p = nullptr;
  if (has_thr) {
    CHECK_IN(threshold.value()); CHECK_IN(threshold_lr.value());
    TORCH_CHECK(threshold->numel() == M && threshold_n->numel() == M && threshold_lr->numel() == M,
                "threshold state must be [M]");
    th_p = threshold->data_ptr<float>();
    thn_p = int32_ptr(*threshold_n, "threshold_n");
    thlr_p = threshold_lr->data_ptr<float>();
  }
  if (M == 0 || B * n == 0) return;

  // a block takes at least 16 elements per thread; about four blocks per CU in all
  const long cap = std::max(1L, 1024 / M);
  dim3 grid((unsigned)std::min(cap, (B * n + BTK_T * 16 - 1) / (BTK_T * 16)), 1, (unsigned)M);
  hipStream_t st = cur_stream();
  TORCH_CHECK(hipMemsetAsync(work_p, 0, sizeof(int) * batch_topk_workspace_size(M), st) == hipSuccess,
              "batch_topk_select: zeroing the workspace failed");
  const float* s_p = scores.data_ptr<float>();
  hipLaunchKernelGGL(k_btk_hist<0>, grid, dim3(BTK_T), 0, st, s_p, ks_p, work_p, (int)B, (int)n);
  hipLaunchKernelGGL(k_btk_hist<1>, grid, dim3(BTK_T), 0, st, s_p, ks_p, work_p, (int)B, (int)n);
  hipLaunchKernelGGL(k_btk_hist<2>, grid, dim3(BTK_T), 0, st, s_p, ks_p, work_p, (int)B, (int)n);
  hipLaunchKernelGGL(k_btk_write, grid, dim3(BTK_T), 0, st, s_p, c_out.data_ptr<float>(),
                     fired.data_ptr<float>(), ks_p, thr_out.data_ptr<float>(), work_p,
                     th_p, thn_p, thlr_p, (int)B, (int)n);
}

void resample(torch::Tensor fired, torch::Tensor new_rows, torch::Tensor enc_scale,
              torch::Tensor W, torch::Tensor mu_w, torch::Tensor nu_w,
              c10::optional<torch::Tensor> dec,
              c10::optional<torch::Tensor> mu_d, c10::optional<torch::Tensor> nu_d,
              c10::optional<torch::Tensor> bias,
              c10::optional<torch::Tensor> mu_b, c10::optional<torch::Tensor> nu_b,
              torch::Tensor counts_out) {
  CHECK_IN(fired); CHECK_IN(new_rows); CHECK_IN(enc_scale);
  CHECK_IN(W); CHECK_IN(mu_w); CHECK_IN(nu_w);
  int M = W.size(0), n = W.size(1), d = W.size(2);
  int n_track = new_rows.size(1);
  float* dec_p = nullptr; float* mud_p = nullptr; float* nud_p = nullptr;
  if (dec.has_value()) {
    CHECK_IN(dec.value()); CHECK_IN(mu_d.value()); CHECK_IN(nu_d.value());
    dec_p = dec->data_ptr<float>();
    mud_p = mu_d->data_ptr<float>();
    nud_p = nu_d->data_ptr<float>();
  }
  float* b_p = nullptr; float* mub_p = nullptr; float* nub_p = nullptr;
  if (bias.has_value()) {
    CHECK_IN(bias.value()); CHECK_IN(mu_b.value()); CHECK_IN(nu_b.value());
    b_p = bias->data_ptr<float>();
    mub_p = mu_b->data_ptr<float>();
    nub_p = nu_b->data_ptr<float>();
  }
  hipLaunchKernelGGL(k_resample, dim3(M), dim3(RSMP_T), 0, cur_stream(),
                     fired.data_ptr<float>(), new_rows.data_ptr<float>(),
                     enc_scale.data_ptr<float>(), W.data_ptr<float>(),
                     mu_w.data_ptr<float>(), nu_w.data_ptr<float>(),
                     dec_p, mud_p, nud_p, b_p, mub_p, nub_p,
                     int32_ptr(counts_out, "counts_out"), n, d, n_track);
}

void lista_bwd_elem(torch::Tensor g_y, c10::optional<torch::Tensor> carry_in,
                    torch::Tensor r, torch::Tensor theta, torch::Tensor x,
                    torch::Tensor x_prev, torch::Tensor mom,
                    torch::Tensor g_r, torch::Tensor carry_out,
                    torch::Tensor g_theta, torch::Tensor g_rho) {
  CHECK_IN(g_y); CHECK_IN(r); CHECK_IN(theta); CHECK_IN(x); CHECK_IN(x_prev);
  CHECK_IN(mom); CHECK_IN(g_r); CHECK_IN(carry_out); CHECK_IN(g_theta); CHECK_IN(g_rho);
  const float* ci = OPT_PTR(carry_in);
  int M = g_y.size(0), B = g_y.size(1), n = g_y.size(2);
  dim3 grid(cdiv(n, LBW_COLS), cdiv(B, LBW_ROWS), M);
  hipLaunchKernelGGL(k_lista_bwd_elem, grid, dim3(LBW_COLS), 0, cur_stream(),
                     g_y.data_ptr<float>(), ci, r.data_ptr<float>(),
                     theta.data_ptr<float>(), x.data_ptr<float>(),
                     x_prev.data_ptr<float>(), mom.data_ptr<float>(),
                     g_r.data_ptr<float>(), carry_out.data_ptr<float>(),
                     g_theta.data_ptr<float>(), g_rho.data_ptr<float>(), B, n);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("set_aligned_tiles", &set_aligned_tiles,
        "process-wide switch: launch the guard-free GEMM kernels on tile-aligned shapes (default on)",
        py::arg("on"));
  m.def("aligned_tiles", &aligned_tiles, "whether tile-aligned launches take the guard-free kernels");
  m.def("row_norms", &row_norms, "dictionary row norms + clamped inverses");
  m.def("transpose_scale", &transpose_scale, "batched [R,C]->[C,R] transpose with row scale");
  m.def("enc_fwd2", &enc_fwd2, "enc forward, pre-transposed operands (all-direct staging)",
        py::arg("xT"), py::arg("WT"), py::arg("bias"), py::arg("c_out"),
        py::arg("loss_parts"), py::arg("fired"), py::arg("mode"),
        py::arg("bk") = 32, py::arg("prio") = false,
        py::arg("dict_sizes") = py::none());
  m.def("gc2", &gc2, "code-grad, pre-transposed operands",
        py::arg("rT"), py::arg("WT"), py::arg("c"), py::arg("l1_alpha"),
        py::arg("gpre"), py::arg("g_bias"),
        py::arg("bk") = 32, py::arg("prio") = false, py::arg("gc_mode") = 0);
  m.def("enc_fwd", &enc_fwd, "fused encoder GEMM + bias + ReLU/TopK/gate (+L1, fired)",
        py::arg("x"), py::arg("Wenc"), py::arg("bias"), py::arg("inv_norms"),
        py::arg("c_out"), py::arg("loss_parts"), py::arg("fired"), py::arg("mode"),
        py::arg("bk") = 32, py::arg("prio") = false, py::arg("bn") = 128,
        py::arg("act_scale") = py::none(), py::arg("act_gain") = py::none(),
        py::arg("u_out") = py::none(), py::arg("dict_sizes") = py::none(),
        py::arg("y_in") = py::none(), py::arg("x_prev") = py::none(),
        py::arg("x_out") = py::none(), py::arg("mom") = py::none());
  m.def("topk_select", &topk_select, "per-row radix top-k + scatter (+fired)",
        py::arg("scores"), py::arg("c_out"), py::arg("fired"), py::arg("ks"));
  m.def("batch_topk_workspace_size", &batch_topk_workspace_size,
        "int32 workspace elements batch_topk_select needs", py::arg("M"));
  m.def("batch_topk_select", &batch_topk_select,
        "batch-level radix top-k (K = k*B per model) + scatter (+fired, threshold state)",
        py::arg("scores"), py::arg("c_out"), py::arg("fired"), py::arg("ks"),
        py::arg("thr_out"), py::arg("work"),
        py::arg("threshold") = py::none(), py::arg("threshold_n") = py::none(),
        py::arg("threshold_lr") = py::none());
  m.def("resample", &resample, "fused dead-neuron resample (K14): rank dead, rewrite rows, zero Adam state",
        py::arg("fired"), py::arg("new_rows"), py::arg("enc_scale"),
        py::arg("W"), py::arg("mu_w"), py::arg("nu_w"),
        py::arg("dec") = py::none(), py::arg("mu_d") = py::none(), py::arg("nu_d") = py::none(),
        py::arg("bias") = py::none(), py::arg("mu_b") = py::none(), py::arg("nu_b") = py::none(),
        py::arg("counts_out"));
  m.def("lista_bwd_elem", &lista_bwd_elem, "fused LISTA backward elementwise pass",
        py::arg("g_y"), py::arg("carry_in"), py::arg("r"), py::arg("theta"),
        py::arg("x"), py::arg("x_prev"), py::arg("mom"), py::arg("g_r"),
        py::arg("carry_out"), py::arg("g_theta"), py::arg("g_rho"));
  m.def("gc_thresh", &gc_thresh, "code-grad through the threshold gate (+gain/scale grads)",
        py::arg("r"), py::arg("Wdec"), py::arg("inv_norms"), py::arg("c"),
        py::arg("u"), py::arg("act_scale"), py::arg("l1_alpha"), py::arg("gpre"),
        py::arg("g_gain"), py::arg("g_scale"),
        py::arg("bk") = 32, py::arg("prio") = false);
  m.def("dec_fwd", &dec_fwd, "fused decoder GEMM - x (+MSE partial)",
        py::arg("c"), py::arg("Wdec"), py::arg("inv_norms"), py::arg("x"),
        py::arg("r_out"), py::arg("loss_parts"),
        py::arg("bk") = 32, py::arg("prio") = false, py::arg("bn") = 128);
  m.def("gc", &gc, "code-gradient GEMM + relu/reverse mask + l1 term (+bias grad)",
        py::arg("r"), py::arg("Wdec"), py::arg("inv_norms"), py::arg("c"),
        py::arg("l1_alpha"), py::arg("gpre"), py::arg("g_bias"),
        py::arg("bk") = 32, py::arg("prio") = false, py::arg("gc_mode") = 0,
        py::arg("bn") = 128, py::arg("accumulate") = true);
  m.def("grad_w", &grad_w, "gw = beta*gw + alpha * P^T Q (batched over M)",
        py::arg("P"), py::arg("Q"), py::arg("gw"), py::arg("alpha"), py::arg("beta"),
        py::arg("bk") = 32, py::arg("prio") = false, py::arg("bn") = 128);
  m.def("project_adam", &project_adam, "renorm-gradient projection + Adam",
        py::arg("W"), py::arg("gw"), py::arg("norms"), py::arg("mu"),
        py::arg("nu"), py::arg("step_no"), py::arg("n_per_model"),
        py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps_adam"),
        py::arg("eps_norm"), py::arg("project"),
        py::arg("w_used") = py::none(), py::arg("clamp_mask") = false,
        py::arg("lr_mult") = py::none());
  m.def("colsum", &colsum, "out[m,j] = alpha * sum_b X[m,b,j] (coalesced column sum)",
        py::arg("X"), py::arg("out"), py::arg("alpha") = 1.0,
        py::arg("absval") = false);
  m.def("bias_adam", &bias_adam, "Adam on bias with L2-norm decay",
        py::arg("bias"), py::arg("g_bias"), py::arg("decay"), py::arg("mu"),
        py::arg("nu"), py::arg("step_no"), py::arg("lr"), py::arg("b1"),
        py::arg("b2"), py::arg("eps_adam"), py::arg("lr_mult") = py::none());
}
