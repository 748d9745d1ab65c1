// logmel_fft<PCM, T>: the round-3/5 log-mel kernel, a 400-point real FFT per frame in LDS.  NOT the default (logmel.hip: the quad-lane kernel
// is); kept selectable (OASR_LOGMEL=fft, fft32) as the A/B partner the quad kernel is measured against and as a cross-check that sums in
// another order.
//
// The dense DFT (logmel_dft.hip) spends 0.55 GFLOP per clip on the fp32 matrix pipe (3.5 us/clip at its peak, 6.7 measured) for a kernel
// whose algorithmic HBM traffic (1.92 MB/clip) needs 0.3 us.  A 400-point real FFT needs ~10 kFLOP per frame = 30 MFLOP per clip:
// a workgroup takes 32 frames of one clip through
//     pack      z[n] = w[2n] x[2n] + i w[2n+1] x[2n+1], n < 200   (a real 400-point transform as a complex 200-point one)
//     stage A   25 x radix-8 over n1 (n = 25 n1 + n2), twiddle W200^(n2 k1)                       -> A[k1][n2]
//     stage B    8 x 25-point DFT over n2 as 5 x 5 (n2 = 5a + b, k2 = c + 5e; twiddle W25^(b c))   -> Z[k1 + 8 k2]
//     unpack    X[k] = (Z[k] + conj Z[200-k]) / 2 - i W400^k (Z[k] - conj Z[200-k]) / 2, k <= 200 -> |X[k]|^2
//     mel       80 triangular filters as sparse rows (391 non-zeros of 16080), log10, per-clip max
// with every stage laid out as (32 frames) x (8 items per pass) over the 256 threads: the lane index is the frame, so all 32
// lanes of a half-wave run the same butterfly on different frames -- no divergence, table reads are broadcasts, and every LDS
// row stride (162 floats of samples, 201 complex / 201 floats per frame) is odd in its access width: conflict-free.  fp32 throughout
// (twiddles rounded once from double): |error| ~ 1e-7 of the frame's amplitude, same as the k-ordered fmaf chains of the MFMA form.
// (frames per workgroup: template parameter T of logmel_fft, 16 for OASR_LOGMEL=fft)
// Its constant tables stay resident in LDS; logmel_tables.h gives their layout (XTAB_*).
#include "logmel_common.h"

namespace {

constexpr int XROW = 201;                     // per-frame row length (complex for Z, float for the power spectrum)

__device__ __forceinline__ void fft8(cf (&v)[8]) {  // forward, natural order in and out
  constexpr float R2 = 0.70710678118654752f;
  const cf a0 = cadd(v[0], v[4]), a1 = csub(v[0], v[4]), a2 = cadd(v[2], v[6]), a3 = csub(v[2], v[6]);
  const cf a4 = cadd(v[1], v[5]), a5 = csub(v[1], v[5]), a6 = cadd(v[3], v[7]), a7 = csub(v[3], v[7]);
  const cf E0 = cadd(a0, a2), E2 = csub(a0, a2), E1 = cadd(a1, mni(a3)), E3 = cadd(a1, pli(a3));
  const cf O0 = cadd(a4, a6), O2 = csub(a4, a6), O1 = cadd(a5, mni(a7)), O3 = cadd(a5, pli(a7));
  const cf w1 = cf{(O1.x + O1.y) * R2, (O1.y - O1.x) * R2};
  const cf w2 = mni(O2);
  const cf w3 = cf{(O3.y - O3.x) * R2, (-O3.x - O3.y) * R2};
  v[0] = cadd(E0, O0);
  v[1] = cadd(E1, w1);
  v[2] = cadd(E2, w2);
  v[3] = cadd(E3, w3);
  v[4] = csub(E0, O0);
  v[5] = csub(E1, w1);
  v[6] = csub(E2, w2);
  v[7] = csub(E3, w3);
}
__device__ __forceinline__ int xsamp_addr(int s) { return s + 2 * (s / HOP); }  // 162 floats between frames: 81 8-byte slots (odd)

// T = frames per workgroup (32: lane = frame over a half wave, 8 item groups, two workgroups per CU; 16: 16 item groups, 43 KiB of LDS,
// three workgroups per CU -- half the serial work per thread in the sample / unpack / mel stages and 12 instead of 8 waves per CU to hide the
// LDS round trips this kernel is bound by, profiles/r03_logmel_fft.txt)
template <typename PCM, int T>
__global__ __launch_bounds__(256, T == 32 ? 2 : 3) void logmel_fft(const PCM* __restrict__ pcm, int n_samples, int n_frames,
                                                     const float* __restrict__ tab,  // [XTAB]: the three stage tables
                                                     int mel_words,                  // words of the mel table (162 + non-zeros)
                                                     int max_span,                   // taps of the widest filter
                                                     float* __restrict__ out, unsigned* __restrict__ clipmax) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NG = 256 / T;                    // item groups: thread (f = tid % T, j0 = tid / T)
  constexpr int TNS = T * HOP + (NFFT - HOP);    // samples of T frames
  constexpr int TR0 = TNS + 2 * (TNS / HOP + 1);
  float* samp = smem;                       // region 0: samples
  cf* cb = (cf*)(smem + ((TR0 + 3) & ~3));  // [T][XROW] complex: A, then Z, then (as floats, same row stride) the power spectrum
  float* pw = (float*)cb;
  float* tw = smem + ((TR0 + 3) & ~3) + 2 * T * XROW;
  const cf* tw200 = (const cf*)tw;
  const float* win = tw + 400;
  const cf* tw400 = (const cf*)(tw + XTAB_OFF_P);
  // 1-D grid, XCD-contiguous: neighbouring frame blocks of a clip run on the same XCD at the same time, so the 128-byte row
  // segments they write (row pitch 12000 B: never line aligned) meet in ONE L2 and leave it as whole lines, and the 240 samples
  // two neighbours share are fetched once
  const int nblk = (n_frames + T - 1) / T;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int b = bid / nblk, f0 = (bid - b * nblk) * T, tid = threadIdx.x;
  const int f = tid & (T - 1), j0 = tid / T;  // lane = frame, NG items per pass
  const PCM* clip = pcm + (long)b * n_samples;

  for (int i = tid; i < (XTAB_OFF_M + mel_words + 3) / 4; i += 256) ((f32x4_t*)tw)[i] = ((const f32x4_t*)tab)[i];  // (XTAB floats allocated)
  // ---- samples of these 32 frames (reflect padding of torch.stft(center=True) at the clip's ends)
  const long s_begin = (long)f0 * HOP - NFFT / 2;
  const bool interior = s_begin >= 0 && s_begin + TNS <= n_samples && ((size_t)(clip + s_begin) & 15) == 0;
  if (interior) {  // (wave-uniform) 16-byte loads; a vector never straddles a hop boundary (160 % 8 == 0), so its floats stay adjacent
    constexpr int PER = 16 / (int)sizeof(PCM);  // 8 int16 / 4 float samples per load
    for (int v = tid; v < TNS / PER; v += 256) {
      const u32x4_t raw = *(const u32x4_t*)(clip + s_begin + (long)v * PER);
      float* dst = samp + xsamp_addr(v * PER);
      if (sizeof(PCM) == 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int w = (int)raw[i];
          *(float2*)(dst + 2 * i) = float2{(float)(short)(w & 0xffff) * (1.0f / 32768.0f), (float)(w >> 16) * (1.0f / 32768.0f)};
        }
      } else {
        *(float2*)dst = float2{__uint_as_float(raw[0]), __uint_as_float(raw[1])};
        *(float2*)(dst + 2) = float2{__uint_as_float(raw[2]), __uint_as_float(raw[3])};
      }
    }
  } else {
    for (int s = tid; s < TNS; s += 256) {
      samp[xsamp_addr(s)] = load_pcm<PCM>(clip, reflect_index(s_begin + s, n_samples));
    }
  }
  __syncthreads();

  // ---- stage A
#pragma unroll 1
  for (int it = 0; it < (25 + NG - 1) / NG; ++it) {
    const int n2 = it * NG + j0;
    if (n2 < 25) {
      cf v[8];
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1) {
        const int n = 25 * n1 + n2, i0 = 2 * n;
        const float2 x = *(const float2*)(samp + xsamp_addr(f * HOP + i0));
        const float w0 = win[i0 <= 200 ? i0 : NFFT - i0], w1 = win[i0 + 1 <= 200 ? i0 + 1 : NFFT - i0 - 1];
        v[n1] = cf{x.x * w0, x.y * w1};
      }
      fft8(v);
      cf* dst = cb + f * XROW + n2;
      dst[0] = v[0];
#pragma unroll
      for (int k1 = 1; k1 < 8; ++k1) dst[k1 * 25] = cmul(v[k1], tw200[n2 * k1]);  // (n2 k1 <= 168)
    }
  }
  __syncthreads();

  // ---- stage B: k1 = j0 (the groups past 7 idle here when NG = 16)
  {
    const int k1 = j0 & 7;
    const bool act = j0 < 8;
    cf a[25];
    const cf* src = cb + f * XROW + k1 * 25;
    if (act) {
#pragma unroll
      for (int i = 0; i < 25; ++i) a[i] = src[i];
    }
    __syncthreads();  // every thread holds its inputs: the rows can be overwritten in natural order
    if (act) {
      cf bm[5][5];  // [b][c]
#pragma unroll
      for (int bb = 0; bb < 5; ++bb) {
        cf y[5];
        dft5(a[bb], a[5 + bb], a[10 + bb], a[15 + bb], a[20 + bb], y);
        bm[bb][0] = y[0];
#pragma unroll
        for (int c = 1; c < 5; ++c) bm[bb][c] = bb == 0 ? y[c] : cmul(y[c], tw200[8 * bb * c]);  // W25^(b c) = W200^(8 b c)
      }
      cf* dst = cb + f * XROW + k1;
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        cf y[5];
        dft5(bm[0][c], bm[1][c], bm[2][c], bm[3][c], bm[4][c], y);
#pragma unroll
        for (int e = 0; e < 5; ++e) dst[8 * (c + 5 * e)] = y[e];
      }
    }
  }
  __syncthreads();

  // ---- unpack + power: every thread first computes its 26 bins of frame f into registers, then (behind a barrier: all reads of
  // the Z rows are done) writes them over the row, as floats
  {
    constexpr int NU = (201 + NG - 1) / NG;
    float pv[NU];
#pragma unroll
    for (int it = 0; it < NU; ++it) {
      const int k = it * NG + j0;
      pv[it] = 0.f;
      if (k <= 200) {
        const cf zk = cb[f * XROW + (k == 200 ? 0 : k)];
        cf zm = cb[f * XROW + (k == 0 ? 0 : 200 - k)];
        zm.y = -zm.y;
        const cf e = cscale(cadd(zk, zm), 0.5f), o = cscale(mni(csub(zk, zm)), 0.5f);
        const cf x = cadd(e, cmul(tw400[k], o));
        pv[it] = x.x * x.x + x.y * x.y;
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NU; ++it) {
      const int k = it * NG + j0;
      if (k <= 200) pw[f * (2 * XROW) + k] = pv[it];
    }
  }
  __syncthreads();

  // ---- mel filters (sparse rows), log10, per-clip max, store
  const int* mel_idx = (const int*)(tw + XTAB_OFF_M);  // [81][2]: first bin, first weight (row 80 carries the total)
  const float* mel_val = tw + XTAB_OFF_M + 162;
  float vmax = -1e30f;
  const int t = f0 + f;
  {
    // this thread's 10 filters (m = 8 it + j0) advance together, one tap per step: 10 independent LDS-read + fma chains in flight
    // instead of one serial chain per filter (each step is two LDS round trips; the filters have 2..14 taps)
    constexpr int NF = NMEL / NG, NH = (NF + 1) / 2;  // filters per thread (m = NG it + j0); they advance in pairs (a, a + NH)
    int lo[NF], p0[NF], cnt[NF];
    float acc[NF];
#pragma unroll
    for (int it = 0; it < NF; ++it) {
      const int m = it * NG + j0;
      lo[it] = mel_idx[2 * m];
      p0[it] = mel_idx[2 * m + 1];
      cnt[it] = mel_idx[2 * m + 3] - p0[it];
      acc[it] = 0.f;
    }
    const float* prow = pw + f * (2 * XROW);
    // filters a and a + NH advance together (two independent chains); the step count of a pair is the widest filter any lane of
    // the wave holds for it (filter width grows with the index)
#pragma unroll
    for (int a = 0; a < NH; ++a) {
      const int a2 = a + NH < NF ? a + NH : a;  // (odd NF: the last one runs alone)
      int n = cnt[a] > cnt[a2] ? cnt[a] : cnt[a2];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) n = max(n, __shfl_xor(n, o, 64));
      n = __builtin_amdgcn_readfirstlane(n);
      for (int i = 0; i < n; i += 4) {  // 16 LDS reads in flight per trip (reads past a filter's end stay inside the row / the table)
        float x0[4], w0[4], x1[4], w1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          x0[u] = prow[lo[a] + i + u];
          w0[u] = mel_val[p0[a] + i + u];
          x1[u] = prow[lo[a2] + i + u];
          w1[u] = mel_val[p0[a2] + i + u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc[a] = (i + u < cnt[a]) ? fmaf(x0[u], w0[u], acc[a]) : acc[a];
          if (a2 != a) acc[a2] = (i + u < cnt[a2]) ? fmaf(x1[u], w1[u], acc[a2]) : acc[a2];
        }
      }
    }
    if (t < n_frames) {
#pragma unroll
      for (int it = 0; it < NF; ++it) {
        const float v = log10f(fmaxf(acc[it], 1e-10f));
        out[((long)b * NMEL + it * NG + j0) * n_frames + t] = v;
        vmax = fmaxf(vmax, v);
      }
    }
  }
  // one ordered-uint atomicMax per workgroup (the tables are dead: their first words carry the four wave maxima)
  vmax = wave_max(vmax);
  __syncthreads();
  if ((tid & 63) == 0) tw[tid >> 6] = vmax;
  __syncthreads();
  if (tid == 0) {
    const float m4 = fmaxf(fmaxf(tw[0], tw[1]), fmaxf(tw[2], tw[3]));
    if (m4 > -1e29f) atomicMax(clipmax + b, f2ord(m4));
  }
}

template <typename PCM, int T>
int launch_fft(const LogmelArgs& a) {
  constexpr int TNS = T * HOP + (NFFT - HOP), TR0 = TNS + 2 * (TNS / HOP + 1);  // as in the kernel: samples | Z rows | tables
  const size_t lds = sizeof(float) * (((TR0 + 3) & ~3) + 2 * T * XROW + XTAB);
  const dim3 grid((unsigned)(cdiv(a.n_frames, T) * a.B));
  static LdsAttrOnce attr;
  const int rc = ensure_dynamic_lds(attr, (const void*)logmel_fft<PCM, T>, (int)lds);
  if (rc) return rc;
  hipLaunchKernelGGL((logmel_fft<PCM, T>), grid, dim3(256), lds, a.stream, (const PCM*)a.pcm, a.n_samples, a.n_frames, a.tab->fft_tab,
                     a.tab->mel_words, a.tab->mel_span, a.out, a.clipmax);
  OASR_LAUNCH_CHECK();
  return OASR_OK;
}

}  // namespace

int launch_logmel_fft(const LogmelArgs& a, int frames_per_wg) {
  if (a.pcm_dtype == 1) return frames_per_wg == 32 ? launch_fft<int16_t, 32>(a) : launch_fft<int16_t, 16>(a);
  return frames_per_wg == 32 ? launch_fft<float, 32>(a) : launch_fft<float, 16>(a);
}
