// Token selection over the vocabulary, the per-step tail of the decoder loops (gfx950): greedy pick, greedy pick under whisper's timestamp
// rules, top-K for beam search and one inverse-CDF draw, all on fp32 logits [rows][ld] with one 256-thread workgroup per row.  The argument
// block (SelectArgs) and the empty-row contract: kernels.h at launch_pick_tokens.  The filter (additive masks + timestamp rules), the
// row statistics and the (value, index) argmax merge are each stated once below and shared by the kernels.
#include "kernels.h"

namespace {

__device__ __forceinline__ float block_reduce(float v, float* red, bool is_max) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = is_max ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return is_max ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
}

// A candidate (value, column); "none yet" is (-inf, INT_MAX).  Among equal values the lower column wins.
struct Best {
  float v;
  int i;
  __device__ __forceinline__ void take(float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
};
// The best candidate of the workgroup, left in every thread (sh: 4 entries of LDS; a caller that reduces in a loop puts a __syncthreads()
// between two calls, this one does not start with one).
__device__ __forceinline__ Best best_block_reduce(Best b, Best* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) b.take(__shfl_xor(b.v, o, 64), __shfl_xor(b.i, o, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = b;
  __syncthreads();
  b = sh[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) b.take(sh[w].v, sh[w].i);
  return b;
}

// Token pick over the vocabulary (the per-step tail of whisper.decoding's GreedyDecoder.update, and gen_pred's argmax,
// train_timestamps.py:1096-1098): one workgroup per row of fp32 logits;
//   x[c] = logits[c] + mask[c] (+ mask2[c])          (additive 0 / -inf suppress masks, optional)
//   tok = argmax_c x[c] (lowest index among equal maxima), logprob = x[tok] - logsumexp(x)
// (reads no history and no token id of its argument block)
__global__ __launch_bounds__(256) void pick_kernel(const SelectArgs a) {
  __shared__ float red[4];
  __shared__ Best sh[4];
  const float* lr = a.logits + (long)blockIdx.x * a.ld;
  Best b{-INFINITY, 0x7fffffff};
  for (int c = threadIdx.x; c < a.V; c += 256) {
    float x = lr[c];
    if (a.mask) x += a.mask[c];
    if (a.mask2) x += a.mask2[c];
    if (x > b.v) {  // strict: keeps the lowest index of this thread's stride
      b.v = x;
      b.i = c;
    }
  }
  b = best_block_reduce(b, sh);
  float sum = 0.f;
  if (a.logprob) {
    for (int c = threadIdx.x; c < a.V; c += 256) {
      float x = lr[c];
      if (a.mask) x += a.mask[c];
      if (a.mask2) x += a.mask2[c];
      sum += __expf(x - b.v);
    }
    sum = block_reduce(sum, red, false);
  }
  if (threadIdx.x == 0) {
    a.tok[blockIdx.x] = b.i == 0x7fffffff ? 0 : b.i;
    // a row without a survivor (every x = -inf): exp(-inf - -inf) above is NaN; the contract is (0, -inf) (kernels.h at launch_pick_tokens)
    if (a.logprob) a.logprob[blockIdx.x] = b.v > -INFINITY ? -__logf(sum) : -INFINITY;
  }
}

// ---- the filtered distribution: greedy pick, beam search and sampling -----------------------------------------------------------------
// whisper.decoding: GreedyDecoder.update takes the argmax of log_softmax(filtered logits); BeamSearchDecoder.update takes, per beam, the
// beam_size + 1 best log-probabilities of it; GreedyDecoder.update at temperature > 0 draws from Categorical(filtered logits / T) and
// scores the draw with the UN-tempered log_softmax.  "Filtered" = SuppressBlank / SuppressTokens (the additive masks) and, in timestamp
// mode (the reference's default for transcribe(), olmoasr/transcribe.py:212), whisper/decoding.py ApplyTimestampRules.apply: the rules are
// a function of the row's sampled history, which lives on the device (int64 [rows, hist_ld], n_hist tokens sampled so far; n_hist < 0: no
// timestamp rules), so the decoder loop needs no host round trip per token.  Column c of row r is masked (-inf) when
//   c == <|notimestamps|>;
//   the last sampled token is a timestamp and  (the one before it too, or there is none)  -> c >= ts_begin   (text must follow a pair)
//                                              (the one before it is text)                -> c <  eot         (a pair must be closed)
//   a timestamp was sampled before: ts_begin <= c < last_ts (+ 1 unless the last token is an unpaired timestamp)   (monotonic, > 0 s)
//   nothing sampled yet: c < ts_begin, and c > ts_begin + max_initial_index when that is >= 0;
// then, on log_softmax of what is left: if logsumexp(timestamp part) > max(text part) every text column is masked too.
struct TsRules {
  bool on, last_was_ts, pen_was_ts, first;
  int ts_begin, eot, no_ts, ts_lo, ts_hi;  // timestamps below ts_lo / above ts_hi are masked
  __device__ __forceinline__ bool dead(int c) const {
    if (!on) return false;
    const bool is_ts = c >= ts_begin;
    bool d = c == no_ts;
    if (last_was_ts) d = d || (pen_was_ts ? is_ts : c < eot);
    if (is_ts) d = d || c < ts_lo || c > ts_hi;
    else d = d || first;
    return d;
  }
};
// The rules of this workgroup's row (all 256 threads call it; sh_last: 4 ints of LDS)
__device__ __forceinline__ TsRules ts_rules(const SelectArgs& a, int* sh_last) {
  TsRules r;
  const int n_hist = a.n_hist, ts_begin = a.ts_begin;
  r.on = n_hist >= 0;
  r.ts_begin = ts_begin;
  r.eot = a.eot;
  r.no_ts = a.no_ts;
  r.last_was_ts = r.pen_was_ts = r.first = false;
  r.ts_lo = -1;
  r.ts_hi = 0x7fffffff;
  if (!r.on) return r;
  const int64_t* h = a.hist ? a.hist + (long)blockIdx.x * a.hist_ld : nullptr;
  // position of the last sampled timestamp (history is at most n_text_ctx tokens)
  int last_pos = -1;
  for (int t = threadIdx.x; t < n_hist; t += 256)
    if (h[t] >= ts_begin) last_pos = t;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) last_pos = max(last_pos, __shfl_xor(last_pos, o, 64));
  if ((threadIdx.x & 63) == 0) sh_last[threadIdx.x >> 6] = last_pos;
  __syncthreads();
  last_pos = max(max(sh_last[0], sh_last[1]), max(sh_last[2], sh_last[3]));
  r.last_was_ts = n_hist >= 1 && h[n_hist - 1] >= ts_begin;
  r.pen_was_ts = n_hist < 2 || h[n_hist - 2] >= ts_begin;
  if (last_pos >= 0) r.ts_lo = (int)h[last_pos] + ((r.last_was_ts && !r.pen_was_ts) ? 0 : 1);
  r.first = n_hist == 0;
  if (r.first && a.max_initial_index >= 0) r.ts_hi = ts_begin + a.max_initial_index;
  return r;
}
// Whether column c survives the masks and the rules; x: its filtered value then.  (A flag and not a -inf sentinel for the caller to test
// again: one wave per SIMD walks a row, so the loops pay for every instruction -- profiles/select_split_ab.txt.)
__device__ __forceinline__ bool alive(const float* lr, const SelectArgs& a, const TsRules& R, int c, float& x) {
  x = lr[c];
  if (a.mask) x += a.mask[c];
  if (a.mask2) x += a.mask2[c];
  return !R.dead(c) && x > -INFINITY;
}

// online (max, sum-exp, argmax) of one part of a row
struct PickPart {
  float m, s;
  int i;
};
__device__ __forceinline__ void pick_merge(PickPart& a, const PickPart& b) {
  if (b.m > a.m || (b.m == a.m && b.i < a.i)) {
    a.s = a.s * __expf(a.m - b.m) + b.s;  // (a.m = -inf: exp(-inf) = 0; both -inf: handled by the caller's guard)
    a.m = b.m;
    a.i = b.i;
  } else if (b.m > -INFINITY) {
    a.s += b.s * __expf(b.m - a.m);
  }
}
__device__ __forceinline__ PickPart pick_block_reduce(PickPart p, PickPart* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    PickPart q;
    q.m = __shfl_xor(p.m, o, 64);
    q.s = __shfl_xor(p.s, o, 64);
    q.i = __shfl_xor(p.i, o, 64);
    pick_merge(p, q);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wave] = p;
  __syncthreads();
  p = sh[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) pick_merge(p, sh[w]);
  return p;
}
// Pass 1 of every rule-aware kernel, one pass over the row: (max, sum-exp, argmax) of the text and the timestamp part -> M = row maximum,
// lse = log sum exp(x - M) over the survivors, text_off = whether the "timestamp mass beats every text token" rule removes the text part
// (M and lse are then the timestamp part's), any = false for an empty row; and the greedy answer: pick = argmax of the survivors (lowest
// index on ties), lp = its log_softmax over the survivors (GreedyDecoder.update).
struct RowStat {
  float M, lse;
  bool text_off, any;
  int pick;
  float lp;
};
__device__ __forceinline__ RowStat row_stat(const float* lr, const SelectArgs& a, const TsRules& R, PickPart* sh) {
  PickPart text{-INFINITY, 0.f, 0x7fffffff}, stamp{-INFINITY, 0.f, 0x7fffffff};
  for (int c = threadIdx.x; c < a.V; c += 256) {
    float x;
    if (!alive(lr, a, R, c, x)) continue;
    PickPart& p = (R.on && c >= R.ts_begin) ? stamp : text;
    if (x > p.m) {  // strict: lowest index of this thread's stride
      p.s = p.s * __expf(p.m - x) + 1.f;
      p.m = x;
      p.i = c;
    } else {
      p.s += __expf(x - p.m);
    }
  }
  text = pick_block_reduce(text, sh);
  stamp = pick_block_reduce(stamp, sh);
  RowStat st;
  st.M = fmaxf(text.m, stamp.m);
  st.any = st.M > -INFINITY;
  st.text_off = false;
  st.lse = 0.f;
  st.pick = 0;
  st.lp = -INFINITY;
  if (st.any) {
    const float wt = text.m > -INFINITY ? text.s * __expf(text.m - st.M) : 0.f;
    const float ws = stamp.m > -INFINITY ? stamp.s * __expf(stamp.m - st.M) : 0.f;
    st.lse = __logf(wt + ws);
    st.text_off = stamp.m > -INFINITY && (text.m == -INFINITY || (__logf(ws) - st.lse) > ((text.m - st.M) - st.lse));
    if (st.text_off) {
      st.pick = stamp.i;
      st.lp = -__logf(stamp.s);  // (not (M - M) - lse: the sign of a zero would differ)
      st.M = stamp.m;
      st.lse = __logf(stamp.s);
    } else {
      const bool from_text = text.m >= stamp.m;  // equal maxima: text ids are the lower ones
      st.pick = from_text ? text.i : stamp.i;
      st.lp = ((from_text ? text.m : stamp.m) - st.M) - st.lse;
    }
  }
  return st;
}

// The greedy pick of the filtered distribution: row_stat's answer, stored.
__global__ __launch_bounds__(256) void pick_ts_kernel(const SelectArgs a) {
  __shared__ PickPart sh[4];
  __shared__ int sh_last[4];
  const TsRules R = ts_rules(a, sh_last);
  const RowStat st = row_stat(a.logits + (long)blockIdx.x * a.ld, a, R, sh);
  if (threadIdx.x == 0) {
    a.tok[blockIdx.x] = st.pick;
    if (a.logprob) a.logprob[blockIdx.x] = st.lp;
  }
}

// K <= 16 best (log_softmax value, token) pairs of each row, descending, ties to the lower token id.  K + 1 passes over the row (it
// stays in L2): pass j finds the best survivor strictly after pick j-1 in (value desc, id asc) order.
__global__ __launch_bounds__(256) void topk_ts_kernel(const SelectArgs a, int K) {
  __shared__ PickPart sh[4];
  __shared__ int sh_last[4];
  __shared__ Best shb[4];
  const float* lr = a.logits + (long)blockIdx.x * a.ld;
  const TsRules R = ts_rules(a, sh_last);
  const RowStat st = row_stat(lr, a, R, sh);
  Best prev{INFINITY, -1};
  for (int j = 0; j < K; ++j) {
    Best b{-INFINITY, 0x7fffffff};
    if (st.any) {
      for (int c = threadIdx.x; c < a.V; c += 256) {
        if (st.text_off && c < R.ts_begin) continue;
        float x;
        if (!alive(lr, a, R, c, x)) continue;
        if (!(x < prev.v || (x == prev.v && c > prev.i))) continue;  // not after the previous pick
        if (x > b.v) {  // (ascending c within a thread: the first of equal values wins)
          b.v = x;
          b.i = c;
        }
      }
    }
    __syncthreads();  // (shb of pass j - 1 has been read)
    b = best_block_reduce(b, shb);
    if (threadIdx.x == 0) {
      const bool ok = b.v > -INFINITY;
      a.tok[(long)blockIdx.x * K + j] = ok ? b.i : 0;
      a.logprob[(long)blockIdx.x * K + j] = ok ? (b.v - st.M) - st.lse : -INFINITY;
    }
    prev = b;
  }
}

// One draw per row from softmax(filtered logits / temperature) by inverse CDF on the caller's uniform u[row] in [0, 1): every thread
// owns a contiguous range of columns, the block scans the range masses, the owner of u * total walks its range.  logprob = the draw's
// log_softmax at temperature 1 (what GreedyDecoder.update accumulates).
__global__ __launch_bounds__(256) void sample_ts_kernel(const SelectArgs a, float inv_temp, const float* __restrict__ u) {
  __shared__ PickPart sh[4];
  __shared__ int sh_last[4];
  __shared__ float part[256];
  __shared__ int pick_sh;
  const int V = a.V;
  const float* lr = a.logits + (long)blockIdx.x * a.ld;
  const TsRules R = ts_rules(a, sh_last);
  const RowStat st = row_stat(lr, a, R, sh);
  const int per = (V + 255) / 256, c0 = threadIdx.x * per, c1 = min(V, c0 + per);
  float mass = 0.f;
  if (st.any)
    for (int c = c0; c < c1; ++c) {
      if (st.text_off && c < R.ts_begin) continue;
      float x;
      if (alive(lr, a, R, c, x)) mass += __expf((x - st.M) * inv_temp);
    }
  part[threadIdx.x] = mass;
  if (threadIdx.x == 0) pick_sh = -1;
  __syncthreads();
  if (threadIdx.x == 0 && st.any) {  // (256 additions: not worth a parallel scan)
    float total = 0.f;
    for (int t = 0; t < 256; ++t) total += part[t];
    const float target = u[blockIdx.x] * total;
    float acc = 0.f;
    int owner = -1, last_nz = -1;
    for (int t = 0; t < 256; ++t) {
      if (part[t] > 0.f) last_nz = t;
      if (owner < 0 && part[t] > 0.f && target < acc + part[t]) owner = t;
      if (owner < 0) acc += part[t];
    }
    if (owner < 0) {  // rounding pushed the target past the end: the last range with any mass
      owner = last_nz;
      acc = total - part[last_nz];
    }
    // walk the owner's range
    const int a0 = owner * per, a1 = min(V, a0 + per);
    int pick = -1, last = -1;
    float run = acc;
    for (int c = a0; c < a1 && pick < 0; ++c) {
      if (st.text_off && c < R.ts_begin) continue;
      float x;
      if (!alive(lr, a, R, c, x)) continue;
      last = c;
      run += __expf((x - st.M) * inv_temp);
      if (target < run) pick = c;
    }
    pick_sh = pick >= 0 ? pick : last;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int pick = pick_sh;
    float x = -INFINITY;
    if (pick >= 0) alive(lr, a, R, pick, x);  // (a survivor: this is its value)
    a.tok[blockIdx.x] = pick >= 0 ? pick : 0;
    if (a.logprob) a.logprob[blockIdx.x] = pick >= 0 ? (x - st.M) - st.lse : -INFINITY;
  }
}

// rules_optional: n_hist < 0 is accepted and means "no timestamp rules" (then neither the history nor the token ids are read)
int check_select_args(const char* who, const SelectArgs& a, bool rules_optional) {
  OASR_REQUIRE(a.logits && a.tok && a.V > 0 && a.ld >= a.V, "%s: bad args", who);
  if (rules_optional && a.n_hist < 0) return OASR_OK;
  OASR_REQUIRE(a.n_hist >= 0 && (a.n_hist == 0 || (a.hist && a.hist_ld >= a.n_hist)) && 0 <= a.eot && a.eot < a.ts_begin && a.ts_begin < a.V,
               "%s: bad history / token ids", who);
  return OASR_OK;
}

}  // namespace

int launch_pick_tokens(const SelectArgs& a, hipStream_t s) {
  if (int e = check_select_args("pick_tokens", a, true)) return e;
  if (a.rows <= 0) return OASR_OK;
  hipLaunchKernelGGL(pick_kernel, dim3((unsigned)a.rows), dim3(256), 0, s, a);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

int launch_pick_tokens_ts(const SelectArgs& a, hipStream_t s) {
  if (int e = check_select_args("pick_tokens_ts", a, false)) return e;
  if (a.rows <= 0) return OASR_OK;
  hipLaunchKernelGGL(pick_ts_kernel, dim3((unsigned)a.rows), dim3(256), 0, s, a);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

int launch_topk_tokens_ts(const SelectArgs& a, int K, hipStream_t s) {
  if (int e = check_select_args("topk_tokens_ts", a, true)) return e;
  OASR_REQUIRE(a.logprob && K >= 1 && K <= 16 && K <= a.V, "topk_tokens_ts: bad args (K=%d)", K);
  if (a.rows <= 0) return OASR_OK;
  hipLaunchKernelGGL(topk_ts_kernel, dim3((unsigned)a.rows), dim3(256), 0, s, a, K);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

int launch_sample_tokens_ts(const SelectArgs& a, float temperature, const float* u, hipStream_t s) {
  if (int e = check_select_args("sample_tokens_ts", a, true)) return e;
  OASR_REQUIRE(u && temperature > 0.f, "sample_tokens_ts: bad args");
  if (a.rows <= 0) return OASR_OK;
  hipLaunchKernelGGL(sample_ts_kernel, dim3((unsigned)a.rows), dim3(256), 0, s, a, 1.0f / temperature, u);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}
