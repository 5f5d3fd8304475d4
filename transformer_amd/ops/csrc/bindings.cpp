// Python bindings for the CDNA4 kernel library (_tfmx_C).
// Kernel semantics are defined by transformer_amd/ops/reference.py; shapes
// and dtypes are validated here so kernels can assume clean inputs.
#include <torch/extension.h>

#include <vector>

// ---- implemented in the .hip translation units ----------------------------
torch::Tensor gemm_nt(torch::Tensor a, torch::Tensor w, torch::Tensor bias,
                      int64_t epilogue, c10::optional<torch::Tensor> out);
torch::Tensor gemm256_nt(torch::Tensor a, torch::Tensor w, torch::Tensor bias,
                         int64_t epilogue, c10::optional<torch::Tensor> out,
                         c10::optional<torch::Tensor> aux);
bool gemm256_viable(int M, int N, int K, int lda, int ldb);
torch::Tensor gemm128_nt(torch::Tensor a, torch::Tensor w, torch::Tensor bias,
                         int64_t epilogue, c10::optional<torch::Tensor> out);
torch::Tensor gemm_dw(torch::Tensor dy, torch::Tensor x,
                      c10::optional<torch::Tensor> out,
                      c10::optional<torch::Tensor> db,
                      c10::optional<torch::Tensor> cw_cached);
torch::Tensor gemm_nn(torch::Tensor a, torch::Tensor b,
                      c10::optional<torch::Tensor> out);
torch::Tensor gemm_tn(torch::Tensor a, torch::Tensor b,
                      c10::optional<torch::Tensor> out);
torch::Tensor transpose2d(torch::Tensor a);
void transpose2d_into(torch::Tensor a, torch::Tensor out);
void transpose_batch(torch::Tensor desc);
torch::Tensor colsum(torch::Tensor a, c10::optional<torch::Tensor> out);
torch::Tensor gemm_uni_nt(torch::Tensor a, torch::Tensor w,
                          c10::optional<torch::Tensor> bias, int64_t epilogue,
                          c10::optional<torch::Tensor> out);
torch::Tensor gemm_uni_nn(torch::Tensor a, torch::Tensor w,
                          c10::optional<torch::Tensor> out);
torch::Tensor gemm_uni_tn(torch::Tensor dy, torch::Tensor x,
                          c10::optional<torch::Tensor> out, int64_t splitr);
bool gemm_uni_viable(int M, int N, int K);
torch::Tensor gemm_uni_nt_ab(torch::Tensor a, torch::Tensor w,
                             int64_t sched);
torch::Tensor relu_bwd(torch::Tensor dy, torch::Tensor y);
std::vector<torch::Tensor> relu_bwd_db(torch::Tensor dy, torch::Tensor y,
                                       c10::optional<torch::Tensor> db_out);
torch::Tensor smoke_add(torch::Tensor a, torch::Tensor b);

std::vector<torch::Tensor> ln_fwd(torch::Tensor x, torch::Tensor res,
                                  torch::Tensor gamma, torch::Tensor beta,
                                  double eps, double p, int64_t seed,
                                  c10::optional<torch::Tensor> seed_t);
std::vector<torch::Tensor> ln_bwd(torch::Tensor dy, torch::Tensor s,
                                  torch::Tensor gamma, torch::Tensor mean,
                                  torch::Tensor rstd,
                                  c10::optional<torch::Tensor> dgamma_out,
                                  c10::optional<torch::Tensor> dbeta_out,
                                  c10::optional<torch::Tensor> mask,
                                  double p,
                                  c10::optional<torch::Tensor> dbias_out);

std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor kv_pad,
                                    bool causal, double scale, int64_t trv);
std::vector<torch::Tensor> attn_bwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor o,
                                    torch::Tensor dout, torch::Tensor lse,
                                    torch::Tensor kv_pad, bool causal,
                                    double scale, int64_t mode);
std::vector<torch::Tensor> attn_fwd_seg(torch::Tensor q, torch::Tensor k,
                                        torch::Tensor v, torch::Tensor q_seg,
                                        torch::Tensor kv_seg, bool causal,
                                        double scale);
std::vector<torch::Tensor> attn_bwd_seg(torch::Tensor q, torch::Tensor k,
                                        torch::Tensor v, torch::Tensor o,
                                        torch::Tensor dout, torch::Tensor lse,
                                        torch::Tensor q_seg,
                                        torch::Tensor kv_seg, bool causal,
                                        double scale, int64_t mode);

torch::Tensor embed_pe_fwd(torch::Tensor tokens, torch::Tensor weight,
                           torch::Tensor pe,
                           c10::optional<torch::Tensor> positions);
torch::Tensor embed_pe_bwd(torch::Tensor dy, torch::Tensor tokens,
                           int64_t vocab,
                           c10::optional<torch::Tensor> out);

std::vector<torch::Tensor> dropout_fwd(torch::Tensor x, double p,
                                        int64_t seed,
                                        c10::optional<torch::Tensor> seed_t);
torch::Tensor dropout_bwd(torch::Tensor dy, torch::Tensor mask, double p);

std::vector<torch::Tensor> ce_fwd(torch::Tensor logits, torch::Tensor targets,
                                  double batch_size, double label_smoothing);
torch::Tensor ce_bwd(torch::Tensor logits, torch::Tensor targets,
                     torch::Tensor lse, torch::Tensor dloss,
                     double batch_size, double label_smoothing);
std::vector<torch::Tensor> ce_fused(torch::Tensor logits,
                                    torch::Tensor targets,
                                    double batch_size,
                                    double label_smoothing);
void ce_scale(torch::Tensor dlogits, torch::Tensor dloss);

void adam_fused_dev(torch::Tensor master, torch::Tensor m, torch::Tensor v,
                    torch::Tensor grad, torch::Tensor param,
                    torch::Tensor step, torch::Tensor coefs, double d_model,
                    double warmup, double beta1, double beta2, double eps);
void adam_fused(torch::Tensor master, torch::Tensor m, torch::Tensor v,
                torch::Tensor grad, torch::Tensor param, double lr,
                double beta1, double beta2, double eps, int64_t step);
void adam_fused_clip(torch::Tensor master, torch::Tensor m, torch::Tensor v,
                     torch::Tensor grad, torch::Tensor param, double lr,
                     double beta1, double beta2, double eps, int64_t step,
                     torch::Tensor stats);
void adam_fused_dev_clip(torch::Tensor master, torch::Tensor m,
                         torch::Tensor v, torch::Tensor grad,
                         torch::Tensor param, torch::Tensor step,
                         torch::Tensor coefs, double d_model, double warmup,
                         double beta1, double beta2, double eps,
                         torch::Tensor stats);
void grad_norm_clip(torch::Tensor grad, torch::Tensor partials,
                    torch::Tensor stats, double max_norm,
                    bool skip_nonfinite);
void grad_norm_clip_f32(torch::Tensor acc, torch::Tensor partials,
                        torch::Tensor stats, double max_norm,
                        bool skip_nonfinite);
int64_t grad_norm_blocks(int64_t n);
void grad_accum(torch::Tensor grad, torch::Tensor acc);
int64_t grad_accum_max_blocks();
void adam_fused_acc(torch::Tensor master, torch::Tensor m, torch::Tensor v,
                    torch::Tensor acc, torch::Tensor param, double lr,
                    double beta1, double beta2, double eps, int64_t step,
                    c10::optional<torch::Tensor> stats);
void adam_fused_dev_acc(torch::Tensor master, torch::Tensor m,
                        torch::Tensor v, torch::Tensor acc,
                        torch::Tensor param, torch::Tensor step,
                        torch::Tensor coefs, double d_model, double warmup,
                        double beta1, double beta2, double eps,
                        c10::optional<torch::Tensor> stats);
int64_t grad_norm_max_blocks();

torch::Tensor argmax_lastdim(torch::Tensor logits);
std::vector<int64_t> accuracy(torch::Tensor logits, torch::Tensor targets);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("gemm_nt", &gemm_nt,
        "C[M,N] = A[M,K] @ W[N,K]^T + bias (epilogue: 0=none 1=relu)",
        pybind11::arg("a"), pybind11::arg("w"), pybind11::arg("bias"),
        pybind11::arg("epilogue"), pybind11::arg("out") = pybind11::none());
  m.def("gemm_dw", &gemm_dw,
        "C[N,K] = dY[M,N]^T @ X[M,K] — deep-contraction dW via tr16 reads; "
        "optional fused bias grad db[N]",
        pybind11::arg("dy"), pybind11::arg("x"),
        pybind11::arg("out") = pybind11::none(),
        pybind11::arg("db") = pybind11::none(),
        pybind11::arg("cw") = pybind11::none());
  m.def("gemm128_nt", &gemm128_nt, "128x128 NT path, no 256 dispatch (A/B)",
        pybind11::arg("a"), pybind11::arg("w"), pybind11::arg("bias"),
        pybind11::arg("epilogue"), pybind11::arg("out") = pybind11::none());
  m.def("gemm256_nt", &gemm256_nt,
        "256x256 deep-pipelined NT GEMM (K%64==0; M/N any, edge-clamped); "
        "epilogue 0=none 1=relu, with aux (M,N): 2=relu-mask (aux>0 ? c : 0) "
        "3=residual-add (c + aux, one rounding)",
        pybind11::arg("a"), pybind11::arg("w"), pybind11::arg("bias"),
        pybind11::arg("epilogue"), pybind11::arg("out") = pybind11::none(),
        pybind11::arg("aux") = pybind11::none());
  m.def("gemm256_viable",
        [](int M, int N, int K) { return gemm256_viable(M, N, K, K, K); },
        "whether gemm_nt dispatches (M,N,K) to the 256-tile kernel");
  m.def("gemm_nn", &gemm_nn, "C[M,N] = A[M,K] @ B[K,N] (dX)",
        pybind11::arg("a"), pybind11::arg("b"),
        pybind11::arg("out") = pybind11::none());
  m.def("gemm_tn", &gemm_tn, "C[M,N] = A[K,M]^T @ B[K,N] (dW)",
        pybind11::arg("a"), pybind11::arg("b"),
        pybind11::arg("out") = pybind11::none());
  m.def("transpose2d", &transpose2d);
  m.def("transpose2d_into", &transpose2d_into,
        "transpose a into out (out rows may be padded past a's row count)");
  m.def("transpose_batch", &transpose_batch,
        "batched 64x64-tile transposes from an int64 descriptor table");
  m.def("gemm_uni_nt", &gemm_uni_nt,
        "deep-pipelined 256-tile NT fwd GEMM (+bias/ReLU)",
        pybind11::arg("a"), pybind11::arg("w"),
        pybind11::arg("bias") = c10::nullopt, pybind11::arg("epilogue") = 0,
        pybind11::arg("out") = c10::nullopt);
  m.def("gemm_uni_nn", &gemm_uni_nn,
        "dX = dY @ W, W read red-major via tr16 (no weight transpose)",
        pybind11::arg("a"), pybind11::arg("w"),
        pybind11::arg("out") = c10::nullopt);
  m.def("gemm_uni_tn", &gemm_uni_tn,
        "dW = dY^T @ X, both operands tr16-read; optional split contraction",
        pybind11::arg("dy"), pybind11::arg("x"),
        pybind11::arg("out") = c10::nullopt, pybind11::arg("splitr") = 1);
  m.def("gemm_uni_viable", &gemm_uni_viable);
  m.def("gemm_uni_nt_ab", &gemm_uni_nt_ab,
        "schedule A/B variants of the uni NT kernel (bench only)");
  m.def("colsum", &colsum,
        "column sums of a row-strided bf16 matrix; row-streaming kernel on "
        "16-byte-aligned inputs, TFMX_COLSUM=cols keeps the column kernel",
        pybind11::arg("a"), pybind11::arg("out") = pybind11::none());
  m.def("relu_bwd", &relu_bwd);
  m.def("relu_bwd_db", &relu_bwd_db,
        "dz = dy*(y>0) and db = colsum(dz) in one row-streaming pass",
        pybind11::arg("dy"), pybind11::arg("y"),
        pybind11::arg("db") = pybind11::none());
  m.def("smoke_add", &smoke_add);
  m.def("ln_fwd", &ln_fwd, pybind11::arg("x"), pybind11::arg("res"),
        pybind11::arg("gamma"), pybind11::arg("beta"), pybind11::arg("eps"),
        pybind11::arg("p") = 0.0, pybind11::arg("seed") = 0,
        pybind11::arg("seed_t") = pybind11::none());
  m.def("ln_bwd", &ln_bwd, pybind11::arg("dy"), pybind11::arg("s"),
        pybind11::arg("gamma"), pybind11::arg("mean"), pybind11::arg("rstd"),
        pybind11::arg("dgamma_out") = pybind11::none(),
        pybind11::arg("dbeta_out") = pybind11::none(),
        pybind11::arg("mask") = pybind11::none(),
        pybind11::arg("p") = 0.0,
        pybind11::arg("dbias_out") = pybind11::none());
  m.def("attn_fwd", &attn_fwd, pybind11::arg("q"), pybind11::arg("k"),
        pybind11::arg("v"), pybind11::arg("kv_pad"), pybind11::arg("causal"),
        pybind11::arg("scale"), pybind11::arg("trv") = 1);
  m.def("attn_bwd", &attn_bwd, pybind11::arg("q"), pybind11::arg("k"),
        pybind11::arg("v"), pybind11::arg("o"), pybind11::arg("dout"),
        pybind11::arg("lse"), pybind11::arg("kv_pad"), pybind11::arg("causal"),
        pybind11::arg("scale"), pybind11::arg("mode") = 0);
  m.def("attn_fwd_seg", &attn_fwd_seg,
        "attn_fwd with int32 segment ids (B,Sq)/(B,Sk), 0 = pad: a query "
        "sees the keys of its own non-zero id only (selection, not -1e9); "
        "tiles outside a block's id range are skipped",
        pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"),
        pybind11::arg("q_seg"), pybind11::arg("kv_seg"),
        pybind11::arg("causal"), pybind11::arg("scale"));
  m.def("attn_bwd_seg", &attn_bwd_seg, pybind11::arg("q"),
        pybind11::arg("k"), pybind11::arg("v"), pybind11::arg("o"),
        pybind11::arg("dout"), pybind11::arg("lse"), pybind11::arg("q_seg"),
        pybind11::arg("kv_seg"), pybind11::arg("causal"),
        pybind11::arg("scale"), pybind11::arg("mode") = 0);
  m.def("embed_pe_fwd", &embed_pe_fwd, pybind11::arg("tokens"),
        pybind11::arg("weight"), pybind11::arg("pe"),
        pybind11::arg("positions") = pybind11::none());
  m.def("embed_pe_bwd", &embed_pe_bwd, pybind11::arg("dy"),
        pybind11::arg("tokens"), pybind11::arg("vocab"),
        pybind11::arg("out") = pybind11::none());
  m.def("dropout_fwd", &dropout_fwd, pybind11::arg("x"), pybind11::arg("p"),
        pybind11::arg("seed"), pybind11::arg("seed_t") = pybind11::none());
  m.def("dropout_bwd", &dropout_bwd);
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("ce_fused", &ce_fused,
        "loss + gradient in one kernel (the grad sweep re-reads L2-hot "
        "rows); seed applied later by ce_scale (no-op at 1.0)");
  m.def("ce_scale", &ce_scale);
  m.def("adam_fused", &adam_fused);
  m.def("adam_fused_dev", &adam_fused_dev,
        "graph-capturable Adam: device step tensor + in-kernel Noam lr");
  m.def("adam_fused_clip", &adam_fused_clip,
        "adam_fused with grad*stats[1]; no store at all when stats[2] != 0");
  m.def("adam_fused_dev_clip", &adam_fused_dev_clip,
        "adam_fused_dev with grad*stats[1]; a skipped step (stats[2] != 0) "
        "still advances the device step tensor");
  m.def("grad_norm_clip", &grad_norm_clip,
        "deterministic two-stage L2 norm of a 1-D bf16 tensor; stats = "
        "{norm, scale, skipped_this_step, skipped_total}",
        pybind11::arg("grad"), pybind11::arg("partials"),
        pybind11::arg("stats"), pybind11::arg("max_norm"),
        pybind11::arg("skip_nonfinite"));
  m.def("grad_norm_blocks", &grad_norm_blocks,
        "stage-1 block count (= workspace elements) for a length-n input");
  m.def("grad_norm_max_blocks", &grad_norm_max_blocks);
  m.def("grad_norm_clip_f32", &grad_norm_clip_f32,
        "grad_norm_clip over a 1-D fp32 tensor (the gradient accumulator)",
        pybind11::arg("acc"), pybind11::arg("partials"),
        pybind11::arg("stats"), pybind11::arg("max_norm"),
        pybind11::arg("skip_nonfinite"));
  m.def("grad_accum", &grad_accum,
        "acc (fp32) += grad (bf16), 1-D, same length; any base alignment",
        pybind11::arg("grad"), pybind11::arg("acc"));
  m.def("grad_accum_max_blocks", &grad_accum_max_blocks);
  m.def("adam_fused_acc", &adam_fused_acc,
        "adam_fused reading the fp32 accumulator, which it zeroes; optional "
        "stats = {norm, scale, skipped, total} scales / vetoes the update",
        pybind11::arg("master"), pybind11::arg("m"), pybind11::arg("v"),
        pybind11::arg("acc"), pybind11::arg("param"), pybind11::arg("lr"),
        pybind11::arg("beta1"), pybind11::arg("beta2"), pybind11::arg("eps"),
        pybind11::arg("step"), pybind11::arg("stats") = pybind11::none());
  m.def("adam_fused_dev_acc", &adam_fused_dev_acc,
        "adam_fused_dev reading the fp32 accumulator, which it zeroes",
        pybind11::arg("master"), pybind11::arg("m"), pybind11::arg("v"),
        pybind11::arg("acc"), pybind11::arg("param"), pybind11::arg("step"),
        pybind11::arg("coefs"), pybind11::arg("d_model"),
        pybind11::arg("warmup"), pybind11::arg("beta1"),
        pybind11::arg("beta2"), pybind11::arg("eps"),
        pybind11::arg("stats") = pybind11::none());
  m.def("argmax_lastdim", &argmax_lastdim);
  m.def("accuracy", &accuracy);
}
