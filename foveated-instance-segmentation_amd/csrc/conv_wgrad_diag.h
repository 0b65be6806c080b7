// Diagnostic instrumentation of the 3x3 class kernel (conv_wgrad.hip).  The shipped library is built WITHOUT -DFS_WGRAD_TRACE: nothing of
// this file reaches the binary then.
//   -DFS_WGRAD_TRACE  (kernel A/B builds only; tools/wgrad_trace.sh) the host half of the phase trace: a stamp buffer per launch before the
//                     kernel, and after it the per-phase averages of every wave's patch rounds 2..5 on stderr.  The device half (WG_STAMP)
//                     stays beside the kernel.
#pragma once
#ifdef FS_WGRAD_TRACE
#include <hip/hip_runtime.h>
#include <cstdio>
#include "common.h"

static long long* g_wgrad_dbg = nullptr;

template <class Args>
static bool wgrad_traced(const Args& a, long nwg) { return nwg <= 4096 && a.patches_per_split >= 6; }

// before the launch: a zeroed stamp buffer in a.dbg (nullptr where the launch is not traced)
template <class Args>
static int wgrad_trace_begin(Args& a, int ntile, int nsplit, hipStream_t stream) {
  long long*& dbg = g_wgrad_dbg;
  const long nwg = (long)ntile * nsplit;
  const bool traced = wgrad_traced(a, nwg);
  if (traced) {
    if (dbg == nullptr && hipMalloc(&dbg, sizeof(long long) * 4096 * 4 * 4 * 8) != hipSuccess) return FS_ERR_ARG;
    if (hipMemsetAsync(dbg, 0, sizeof(long long) * nwg * 4 * 4 * 8, stream) != hipSuccess) return FS_ERR_ARG;
  }
  a.dbg = traced ? dbg : nullptr;
  return FS_OK;
}

// after the launch: wait for it and print what the stamps say
template <class Args>
static int wgrad_trace_report(const Args& a, int ntile, int nsplit, hipStream_t stream) {
  long long* const dbg = g_wgrad_dbg;
  const long nwg = (long)ntile * nsplit;
  const bool traced = wgrad_traced(a, nwg);
  if (traced) {
    static long long host[4096 * 4 * 4 * 8];
    if (hipStreamSynchronize(stream) != hipSuccess || hipMemcpy(host, dbg, sizeof(long long) * nwg * 128, hipMemcpyDeviceToHost) != hipSuccess) return FS_ERR_ARG;
    // phases: [0->1] address + issue loads, [1->2] barrier (partners still multiplying), [2->3] loads landed, [3->4] split + LDS stores,
    // [4->5] barrier, [5->6] MFMA loop, [6->0'] loop overhead to the next round's top; per wave, rounds 2..4 (round 5 has no successor stamp)
    double sum[8] = {0}, skew_mfma = 0, round_len = 0; long n = 0, nr = 0;
    double par_mfma[2] = {0, 0}, par_round[2] = {0, 0}, par_start[2] = {0, 0}; long par_n[2] = {0, 0};
    long long tmin = 0;
    for (long w_ = 0; w_ < nwg; ++w_) { const long long v = host[(w_ * 4 * 4) * 8]; if (v != 0 && (tmin == 0 || v < tmin)) tmin = v; }
    for (long w_ = 0; w_ < nwg; ++w_) {
      for (int it = 0; it < 3; ++it) {
        long long end_min = 0, end_max = 0;
        for (int wv = 0; wv < 4; ++wv) {
          const long long* t = host + ((w_ * 4 + wv) * 4 + it) * 8;
          const long long* tn = t + 8;
          if (t[0] == 0 || t[6] == 0 || tn[0] == 0) continue;
          for (int i = 0; i < 6; ++i) sum[i] += (double)(t[i + 1] - t[i]);
          sum[6] += (double)(tn[0] - t[6]);
          round_len += (double)(tn[0] - t[0]);
          {
            const int par = (int)((unsigned)host[((w_ * 4 + wv) * 4) * 8 + 7] & 1u);
            par_mfma[par] += (double)(t[6] - t[5]); par_round[par] += (double)(tn[0] - t[0]); ++par_n[par];
            if (it == 0) par_start[par] += (double)(t[0] - tmin);
          }
          ++n;
          if (wv == 0 || t[6] < end_min) end_min = t[6];
          if (wv == 0 || t[6] > end_max) end_max = t[6];
        }
        skew_mfma += (double)(end_max - end_min); ++nr;
      }
    }
    {
      long hist[16] = {0}; long same = 0, pairs = 0;
      static int cu_slot[8][16][16][4];      // [xcc guess = wg % 8][se][cu][simd] -> last wave_id seen
      for (auto& a0 : cu_slot) for (auto& a1 : a0) for (auto& a2 : a1) for (int& v : a2) v = -1;
      for (long w_ = 0; w_ < nwg; ++w_)
        for (int wv = 0; wv < 4; ++wv) {
          const unsigned id = (unsigned)host[((w_ * 4 + wv) * 4) * 8 + 7];
          const int wid = id & 15, simd = (id >> 4) & 3, cu = (id >> 8) & 15, se = (id >> 13) & 7;
          ++hist[wid];
          int& prev = cu_slot[w_ % 8][se][cu][simd];
          if (prev >= 0) { ++pairs; if ((prev & 1) == (wid & 1)) ++same; }
          prev = wid;
        }
      fprintf(stderr, "wgrad trace: wave_id histogram");
      for (int i = 0; i < 16; ++i) if (hist[i]) fprintf(stderr, " %d:%ld", i, hist[i]);
      fprintf(stderr, " | SIMDs with two traced waves %ld, of them with EQUAL slot parity %ld\n", pairs, same);
    }
    if (n > 0) {
      fprintf(stderr, "wgrad trace B%d %dx%d %d->%d patches/split %d grid %ld: round %.0f cyc =", a.B, a.H, a.W, a.Cin, a.Cout, a.patches_per_split, nwg, round_len / n);
      const char* nm[7] = {"issue", "barrier1", "loads", "split", "barrier2", "mfma", "next"};
      for (int i = 0; i < 7; ++i) fprintf(stderr, " %s %.0f", nm[i], sum[i] / n);
      fprintf(stderr, " | spread of the four waves' MFMA-loop ends %.0f", skew_mfma / nr);
      for (int par = 0; par < 2; ++par)
        if (par_n[par]) fprintf(stderr, " | slot %d: mfma %.0f round %.0f round-2 top at +%.0f", par, par_mfma[par] / par_n[par], par_round[par] / par_n[par], par_start[par] * 3 / par_n[par]);
      fprintf(stderr, "\n");
    }
  }
  return FS_OK;
}
#endif
