// The engine's GEMM calls: every launch_gemm of the schedules fills its arguments here -- forward products, data gradients, weight gradients
// (split as train_plan.h says), the conv stem's rank-B corrections -- on the stream the runner is launching on (engine_side.h).
#pragma once
#include "engine_side.h"
#include "train_plan.h"

namespace {

template <typename T>
struct GemmCalls : SideStreams {
  typedef OperandViewT<T> View;
  typedef GemmArgsT<T> Gemm;
  using SideStreams::SideStreams;
  float* cs_scratch = nullptr;  // partial rows of fused bias-gradient column sums (GemmArgs.colsum_scratch)
  float* lora_dw = nullptr;     // adapter contexts, backward: Plan::lora_dw
  // where the weight gradient of the tensor at `off` goes: its arena range, or -- an adapted base weight, frozen -- its workspace scratch
  float* Gw(int64_t off) const {
    const int j = c->lora_at(off);
    return j >= 0 ? lora_dw + c->lora[j].dw : c->G(off);
  }

  // out[M,N] (row stride ldc) = act(x[M,K] . W[N,K]^T + bias): what every forward product sets; the caller adds what is its own and launches
  Gemm product(const View& x, long M, int K, const T* W, int N, const float* bias, int act, T* out, T* out_pre, long ldc) const {
    Gemm g = gemm_defaults_t<T>();
    g.A = x;
    g.B = plain_view(W, K);
    g.M = (int)M;
    g.N = N;
    g.K = K;
    g.bias = bias;
    g.act = act;
    g.out = out;
    g.out_pre = out_pre;
    g.ldc = ldc;
    return g;
  }
  int linear(const T* x, long M, int K, const T* W, int N, const float* bias, int act, const T* resid, T* out, T* out_pre) {
    Gemm g = product(plain_view(x, K), M, K, W, N, bias, act, out, out_pre, N);
    g.resid = resid;
    g.ldr = N;
    return launch_gemm(g, st);
  }
  // dx[M,K] = dy[M,N] . W[N,K]  (* gelu'(u))  (+ resid)
  int dgrad(const T* dy, long M, int N, const T* W, int K, const T* dgelu_u, const T* resid, T* dx, float* colsum = nullptr,
            bool u_is_deriv = false) {
    Gemm g = gemm_defaults_t<T>();
    g.A = plain_view(dy, N);
    g.B = plain_view(W, K);
    g.tb = 1;
    g.M = (int)M;
    g.N = K;
    g.K = N;
    g.dgelu_u = dgelu_u;
    g.dgelu_deriv = u_is_deriv ? 1 : 0;
    g.ldu = K;
    g.resid = resid;
    g.ldr = K;
    g.out = dx;
    g.ldc = K;
    g.colsum = colsum;
    g.colsum_scratch = colsum ? cs_scratch : nullptr;
    return launch_gemm(g, st);
  }
  // dW[N,K] (row stride ldw) += alpha * dy[M,N]^T . x[M,K], fp32 atomics
  Gemm outer(const T* dy, long ldy, long M, int N, const View& x, int K, float* dW, long ldw) const {
    Gemm g = gemm_defaults_t<T>();
    g.A = plain_view(dy, ldy);
    g.ta = 1;
    g.B = x;
    g.tb = 1;
    g.M = N;
    g.N = K;
    g.K = (int)M;
    g.out_f32 = dW;
    g.ldc32 = ldw;
    g.atomic = 1;
    return g;
  }
  // a weight gradient over the M token rows, split over them as train_wgrad_plan says
  int wgrad(const T* dy, long ldy, long M, int N, const View& x, int K, float* dW, long ldw) {
    Gemm g = outer(dy, ldy, M, N, x, K, dW, ldw);
    const WgradPlan w = train_wgrad_plan(M, N, K, x.rpb != 0);
    g.split_k = w.split_k;
    g.atomic_on_pp = w.atomic_on_pp;
    return launch_gemm(g, st);
  }
  // The conv weight gradients read their im2col matrix as a plain matrix of overlapping rows, which is wrong in one tap of one window per
  // sample (the tap that should see the zero padding sees the neighbouring sample or a guard row).  That rank-`n` term is taken out again:
  // dW -= dy^T . x over the n rows (one per sample, strides ldy / ldx) of dY and of what those windows wrongly saw.
  int wgrad_uncount(const T* dy, long ldy, int n, int N, const T* x, long ldx, int K, float* dW, long ldw) {
    Gemm g = outer(dy, ldy, n, N, plain_view(x, ldx), K, dW, ldw);
    g.alpha = -1.0f;
    return launch_gemm(g, st);
  }
  // a weight gradient of the decoder backward: on the side stream when the span step asks for it (SIDE_WGRAD), behind everything launched so far
  int wgrad_side(const T* dy, long ldy, long M, int N, const View& x, int K, float* dW, long ldw) {
    if (!(side_mode & SIDE_WGRAD)) return wgrad(dy, ldy, M, N, x, K, dW, ldw);
    RC(fork_to(c->side.stream));
    OnStream on(st, c->side.stream);
    side_pending = true;
    return wgrad(dy, ldy, M, N, x, K, dW, ldw);
  }
  // A weight gradient over consecutive [rows x K] tensors of the arena that one GEMM fills (q|k|v, cross k|v): one launch when all are
  // trainable, one per trainable tensor otherwise (columns j*rows.. of dy).
  // An adapted tensor's gradient goes to its scratch (Gw), so it always gets a launch of its own.
  // `here`: the launches stay on the stream the runner is on (the caller has put it where they belong); else each one may fork to the side stream.
  int wgrad_parts(const T* dy, long ldy, long M, const View& x, int K, const int64_t* offs, int n, int rows, bool here = false) {
    auto go = [&](const T* dy_j, int N, float* dW) { return here ? wgrad(dy_j, ldy, M, N, x, K, dW, K) : wgrad_side(dy_j, ldy, M, N, x, K, dW, K); };
    int ntr = 0;
    for (int j = 0; j < n; ++j) ntr += (c->tr(offs[j]) && c->lora_at(offs[j]) < 0) ? 1 : 0;
    if (ntr == n) return go(dy, n * rows, c->G(offs[0]));
    for (int j = 0; j < n; ++j)
      if (c->wn(offs[j])) RC(go(dy + (long)j * rows, rows, Gw(offs[j])));
    return OASR_OK;
  }
};

}  // namespace
