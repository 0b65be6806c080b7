// The connected component of a bit mask under the gaze (fs_mask_component; no counterpart in the reference: UNPINNED, a definition of
// this library's).  All of it is integer work on bit words (mask_words.h: the layout).  Passes, one workgroup per image each:
//   seed   one pass over the words: the popcount of the mask, and the set pixel nearest to the gaze pixel as the minimum of
//          mask_near_key.  Shuffles in the wave, LDS across the waves, one lane writes comp and the seed record.  No atomics.
//   grow   the hot pass: the reached set R starts as the seed bit and grows inside the mask M until a sweep changes no word.  A sweep
//          is (a) every thread walking a vertical strip -- one word column over a run of rows, down then up, the reached word above
//          carried in a register -- and (b) every thread walking a run of words along a row, right then left, carrying bit 31 / bit 0
//          over the word borders.  Inside a word the fill is bit-parallel (five doubling steps a direction).  R lives in LDS where the
//          image's words fit it, in the output words themselves otherwise; M is re-read from global memory (L2-resident).
// The walks of one pass run side by side and read words their neighbours are writing: R only ever gains bits that belong to the
// component, so whichever value a read sees is a subset of it, and a sweep in which no thread changed a word has read final values
// everywhere -- R is then closed under the step relation inside M, i.e. the component.  The result is a set function of the input:
// the same bits whatever the order of the walks.
#include "mask_words.h"

namespace {

constexpr int COMP_THREADS = 1024;
constexpr long COMP_LDS_WORDS = 39936;                 // R in LDS: 156 KiB of the workgroup's 160, the rest is the static reductions'
constexpr int COMP_MIN_ROWS = 32, COMP_MIN_WORDS = 8; // the shortest strip of pass (a) and run of pass (b), where the image has as many
constexpr int COMP_REC = 4;                            // ints of scratch per image: seed_y, seed_x (-1, -1: none), the grow pass's sweeps (a diagnostic of tools/component_bench.py, no part of the ABI), 1 spare

// every bit of m joined to a bit of s by a run of set bits of m, in both directions (s within m)
__device__ __forceinline__ unsigned int comp_fill(unsigned int s, unsigned int m) {
  unsigned int a = s, ma = m;                          // towards bit 31
  a |= ma & (a << 1);  ma &= ma << 1;
  a |= ma & (a << 2);  ma &= ma << 2;
  a |= ma & (a << 4);  ma &= ma << 4;
  a |= ma & (a << 8);  ma &= ma << 8;
  a |= ma & (a << 16);
  unsigned int mb = m;                                 // towards bit 0
  a |= mb & (a >> 1);  mb &= mb >> 1;
  a |= mb & (a >> 2);  mb &= mb >> 2;
  a |= mb & (a >> 4);  mb &= mb >> 4;
  a |= mb & (a >> 8);  mb &= mb >> 8;
  a |= mb & (a >> 16);
  return a;
}

// comp[b] = (seed_y, seed_x, d2, area_all) or (-1, -1, -1, area_all); rec[b] = (seed_y, seed_x, 0, 0)
__global__ __launch_bounds__(COMP_THREADS) void component_seed_kernel(const unsigned int* __restrict__ bits, const float* __restrict__ focus,
                                                                      long long* __restrict__ comp, int* __restrict__ rec, int Hs, int Ws, int P,
                                                                      long long snap2) {
  __shared__ unsigned long long red_k[COMP_THREADS / 64];
  __shared__ long long red_a[COMP_THREADS / 64];
  const size_t b = blockIdx.x;
  const int py = mask_gaze_px(mask_gaze16(focus[2 * b], Hs)), px = mask_gaze_px(mask_gaze16(focus[2 * b + 1], Ws));
  const int words = Hs * P;
  const unsigned int* mb = bits + b * (size_t)words;
  unsigned long long key = ~0ull;
  long long area = 0;
  for (int i = threadIdx.x; i < words; i += COMP_THREADS) {
    const int y = i / P, c = i - y * P;
    const unsigned int m = mb[i] & mask_tail(c, P, Ws);
    if (m == 0u) continue;
    area += __popc(m);
    key = mask_near_key(key, m, y, c, py, px, Ws);
  }
  key = mask_key_wave_min(key);
  area = wave_sum_ll(area);
  if ((threadIdx.x & 63) == 0) { red_k[threadIdx.x >> 6] = key; red_a[threadIdx.x >> 6] = area; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int i = 1; i < COMP_THREADS / 64; ++i) {
    key = red_k[i] < key ? red_k[i] : key;
    area += red_a[i];
  }
  long long sy = -1, sx = -1, d2 = -1;
  if (area != 0 && (long long)(key >> 31) <= snap2) {
    const long long at = (long long)(key & 0x7fffffffull);
    d2 = (long long)(key >> 31), sy = at / Ws, sx = at - sy * Ws;
  }
  long long* o = comp + b * 4;
  o[0] = sy, o[1] = sx, o[2] = d2, o[3] = area;
  int* r = rec + b * COMP_REC;
  r[0] = (int)sy, r[1] = (int)sx, r[2] = 0, r[3] = 0;
}

// R's words are read and written by many threads between two barriers: relaxed atomics of workgroup scope (plain ds / global
// instructions) keep every access a whole word and keep the compiler from reusing one
__device__ __forceinline__ unsigned int comp_ld(const unsigned int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void comp_st(unsigned int* p, unsigned int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// IN_LDS: R (Hs rows of `pitch` words, pitch odd so that the row walks of pass (b) spread over the banks) is dynamic LDS and is
// stored to out at the end.  Otherwise R is out itself (pitch = P): one workgroup owns the image, and __syncthreads() with its
// workgroup-scope fence orders the words between the passes.  rpr = rows a strip of pass (a) covers, wpr = words a run of pass (b).
template <bool IN_LDS, int CONN>
__global__ __launch_bounds__(COMP_THREADS) void component_grow_kernel(const unsigned int* __restrict__ bits, int* __restrict__ rec,
                                                                      unsigned int* __restrict__ out, int Hs, int Ws, int P, int pitch, int rpr,
                                                                      int wpr) {
  extern __shared__ __attribute__((aligned(16))) unsigned int comp_lds[];
  const size_t b = blockIdx.x;
  const int words = Hs * P;
  const unsigned int* mb = bits + b * (size_t)words;
  unsigned int* ob = out + b * (size_t)words;
  unsigned int* R = IN_LDS ? comp_lds : ob;
  const int sy = rec[b * COMP_REC], sx = rec[b * COMP_REC + 1];
  if (sy < 0) {                                        // no component: all 0 (uniform over the workgroup)
    for (int i = threadIdx.x; i < words; i += COMP_THREADS) ob[i] = 0u;
    return;
  }
  const int rwords = Hs * pitch;
  const int seed_at = sy * pitch + (sx >> 5);
  for (int i = threadIdx.x; i < rwords; i += COMP_THREADS) comp_st(R + i, i == seed_at ? 1u << (sx & 31) : 0u);
  __syncthreads();
  const int strips = (Hs + rpr - 1) / rpr, runs = (P + wpr - 1) / wpr;
  const int items_a = strips * P, items_b = Hs * runs;
  int any, sweeps = 0;
  do {
    int changed = 0;
    ++sweeps;
    // (a) vertical strips: item = strip * P + c, so that a wave's lanes take neighbouring word columns of one strip.  (Reading eight
    // rows ahead and stepping through them in registers was measured slower, 877 against 787 us on the head's own 1024^2 mask:
    // profiles/r23.)
    for (int dir = 0; dir < 2; ++dir) {
      for (int item = threadIdx.x; item < items_a; item += COMP_THREADS) {
        const int strip = item / P, c = item - strip * P;
        const int y0 = strip * rpr, y1 = min(y0 + rpr, Hs);
        const unsigned int tail = mask_tail(c, P, Ws);
        const int step = dir == 0 ? 1 : -1;
        int y = dir == 0 ? y0 : y1 - 1;
        int yp = y - step;                             // the row the walk comes from; outside the image it is background
        unsigned int above = (yp >= 0 && yp < Hs) ? comp_ld(R + yp * pitch + c) : 0u;
        for (int n = y1 - y0; n > 0; --n, yp = y, y += step) {
          unsigned int a = above;
          if (CONN == 8) {
            a |= a << 1 | a >> 1;
            if (yp >= 0 && yp < Hs) {
              if (c > 0) a |= comp_ld(R + yp * pitch + c - 1) >> 31;
              if (c < P - 1) a |= comp_ld(R + yp * pitch + c + 1) << 31;
            }
          }
          const unsigned int r = comp_ld(R + y * pitch + c);
          above = r;
          if (a == 0u) continue;
          const unsigned int m = mb[y * P + c] & tail;
          unsigned int v = r | (m & a);
          if (v != r) {
            v = comp_fill(v, m);
            comp_st(R + y * pitch + c, v);
            changed = 1;
            above = v;
          }
        }
      }
      __syncthreads();
    }
    // (b) runs of words along a row: item = y * runs + run
    for (int dir = 0; dir < 2; ++dir) {
      for (int item = threadIdx.x; item < items_b; item += COMP_THREADS) {
        const int y = item / runs, run = item - y * runs;
        const int c0 = run * wpr, c1 = min(c0 + wpr, P);
        const int step = dir == 0 ? 1 : -1;
        int c = dir == 0 ? c0 : c1 - 1;
        const int cp = c - step;
        unsigned int carry = 0u;                       // the neighbour's border bit, moved to this word's border
        if (cp >= 0 && cp < P) {
          const unsigned int w = comp_ld(R + y * pitch + cp);
          carry = dir == 0 ? w >> 31 : (w & 1u) << 31;
        }
        for (int n = c1 - c0; n > 0; --n, c += step) {
          const unsigned int r = comp_ld(R + y * pitch + c);
          unsigned int v = r;
          if ((dir == 0 && r != 0u) || carry != 0u) {               // the walk to the right fills every word once; the way back only what a carry adds to
            const unsigned int m = mb[y * P + c] & mask_tail(c, P, Ws);
            v = r | (m & carry);
            if (v != 0u && (dir == 0 || v != r)) v = comp_fill(v, m);
            if (v != r) {
              comp_st(R + y * pitch + c, v);
              changed = 1;
            }
          }
          carry = dir == 0 ? v >> 31 : (v & 1u) << 31;
        }
      }
      __syncthreads();
    }
    any = __syncthreads_or(changed);
  } while (any);
  if (threadIdx.x == 0) rec[b * COMP_REC + 2] = sweeps;  // a diagnostic: the last sweep is the one that changed nothing
  if (IN_LDS) {
    for (int i = threadIdx.x; i < words; i += COMP_THREADS) {
      const int y = i / P, c = i - y * P;
      ob[i] = comp_lds[y * pitch + c];
    }
  }
}

}  // namespace

ComponentPlan component_plan(int B, int Hs, int Ws) {
  ComponentPlan p = {};
  // sides: d2 < 2^29, key < 2^60; pixel indices are ints, and the key keeps them in 31 bits
  if (!(B > 0 && Hs > 0 && Ws > 0 && Hs <= MASK_MAX_SIDE && Ws <= MASK_MAX_SIDE && (long)Hs * Ws < MASK_INT_LIMIT)) return p;
  p.P = mask_row_words(Ws);
  const long pitch = p.P | 1;
  p.in_lds = (long)Hs * pitch <= COMP_LDS_WORDS;
  p.pitch = (int)(p.in_lds ? pitch : p.P);
  // pass (a): as many strips a word column as the threads allow, but of COMP_MIN_ROWS rows or more -- a walk carries the set along
  // its whole strip in one pass, across a strip border it takes the next sweep; pass (b) likewise with runs of words along a row
  const long strips = COMP_THREADS / p.P > 0 ? COMP_THREADS / p.P : 1, runs = COMP_THREADS / Hs > 0 ? COMP_THREADS / Hs : 1;
  const long rpr = (Hs + strips - 1) / strips, wpr = (p.P + runs - 1) / runs;
  p.rpr = (int)(rpr > COMP_MIN_ROWS ? rpr : (Hs < COMP_MIN_ROWS ? Hs : COMP_MIN_ROWS));
  p.wpr = (int)(wpr > COMP_MIN_WORDS ? wpr : (p.P < COMP_MIN_WORDS ? p.P : COMP_MIN_WORDS));
  p.scratch = (long)B * COMP_REC;
  p.ok = true;
  return p;
}

// seed then grow; the caller has checked its pointers and p.ok
int component_launch(const ComponentPlan& p, const unsigned int* bits, const float* focus, unsigned int* out, long long* comp, int* scratch,
                     int B, int Hs, int Ws, int conn, long snap2, hipStream_t stream) {
  hipLaunchKernelGGL(component_seed_kernel, dim3((unsigned)B), dim3(COMP_THREADS), 0, stream, bits, focus, comp, scratch, Hs, Ws, p.P,
                     (long long)snap2);
  FS_LAUNCH_CHECK();
  const int lds = p.in_lds ? Hs * p.pitch * (int)sizeof(unsigned int) : 0;
  auto kernel = p.in_lds ? (conn == 8 ? component_grow_kernel<true, 8> : component_grow_kernel<true, 4>)
                         : (conn == 8 ? component_grow_kernel<false, 8> : component_grow_kernel<false, 4>);
  if (lds > 48 * 1024) {
    // beyond the default: a per-device attribute of each kernel, set once -- to the largest size the plan ever asks for, not to this
    // shape's, so that a larger image later in the process is covered by it
    static unsigned long long done8 = 0ull, done4 = 0ull;
    FS_TRY(fs_lds_opt_in(reinterpret_cast<const void*>(kernel), (int)(COMP_LDS_WORDS * sizeof(unsigned int)), conn == 8 ? done8 : done4));
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(COMP_THREADS), (size_t)lds, stream, bits, scratch, out, Hs, Ws, p.P, p.pitch, p.rpr, p.wpr);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

extern "C" {

long fs_mask_component_scratch_ints(int B, int Hs, int Ws) { return component_plan(B, Hs, Ws).scratch; }
// where the grow pass keeps the reached set for this shape: 1 = LDS, 2 = the output words in global memory, 0 = not launchable
int fs_mask_component_route(int B, int Hs, int Ws) {
  const ComponentPlan p = component_plan(B, Hs, Ws);
  return p.ok ? (p.in_lds ? 1 : 2) : 0;
}

int fs_mask_component(const unsigned int* bits, const float* focus, unsigned int* out, long long* comp, int* scratch, int B, int Hs, int Ws,
                      int conn, long snap2, hipStream_t stream) {
  const ComponentPlan p = component_plan(B, Hs, Ws);
  FS_REQUIRE(bits && focus && out && comp && scratch && out != bits && (conn == 4 || conn == 8) && snap2 >= 0 && p.ok);
  return component_launch(p, bits, focus, out, comp, scratch, B, Hs, Ws, conn, snap2, stream);
}

}  // extern "C"
