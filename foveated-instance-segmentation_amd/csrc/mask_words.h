// The bit-word mask layout and the gaze pixel, for every pass over packed masks.
//   layout  a mask of Ws columns is P = ceil(Ws / 32) words a row, rows and images packed: word g of a tensor is word g % P of row
//           g / P = b * Hs + y.  Pixel (y, x) is bit x & 31 of word x >> 5 of its row.  The bits of the last word at x >= Ws are padding:
//           undefined on input, masked by the reader (mask_tail); what a pass stores there is that pass's statement.
//   gaze    a gaze coordinate f in [0, 1] is taken in 1/16 pixel (mask_gaze16) and its pixel is the nearest one (mask_gaze_px).  The
//           gate, the component, the candidate choice and the drawn marker mean the same pixel because they call the same two functions.
// tests/*_ref.py restate these definitions in numpy on purpose: they are the independent side.
#pragma once
#include "common.h"

__host__ __device__ __forceinline__ int mask_row_words(int Ws) { return (Ws + 31) >> 5; }          // P, for Ws > 0

// ---- device --------------------------------------------------------------------------------------------------------------------------
// the gaze coordinate in 1/16-pixel units: clamp(rint((double)f * ((side - 1) * 16)), 0, (side - 1) * 16), NaN -> 0 (both comparisons
// are false for it)
__device__ __forceinline__ long long mask_gaze16(float f, int side) {
  const double top = (double)(((long long)side - 1) * 16);
  double v = rint(__dmul_rn((double)f, top));
  v = v > 0.0 ? v : 0.0;
  v = v < top ? v : top;
  return (long long)v;
}
__device__ __forceinline__ int mask_gaze_px(long long gaze16) { return (int)((gaze16 + 8) >> 4); }

__device__ __forceinline__ unsigned int mask_tail(int c, int P, int Ws) {          // the bits of word column c that are pixels
  return (c == P - 1 && (Ws & 31)) ? (1u << (Ws & 31)) - 1u : 0xffffffffu;
}

// 32 bits of a row's stream of pixels from bit position `bit` (any int: what lies outside the P words is 0).  TAIL: the row is input,
// its padding is masked and what lies outside the Ws pixels is 0; otherwise the words are taken as they are (Ws is not read).
template <bool TAIL>
__device__ __forceinline__ unsigned int mask_window(const unsigned int* row, int P, int Ws, int bit) {
  const int w = bit >> 5, s = bit & 31;                // floor and remainder, also for a negative position
  const unsigned int lo = (w >= 0 && w < P) ? row[w] & (TAIL ? mask_tail(w, P, Ws) : 0xffffffffu) : 0u;
  if (s == 0) return lo;
  const unsigned int hi = (w + 1 >= 0 && w + 1 < P) ? row[w + 1] & (TAIL ? mask_tail(w + 1, P, Ws) : 0xffffffffu) : 0u;
  return (lo >> s) | (hi << (32 - s));
}

// pixel x of a row, `word` being word x >> 5 of that row (the passes address it their own ways: a hoisted column, a shared index)
__device__ __forceinline__ unsigned int mask_bit(unsigned int word, int x) { return (word >> (x & 31)) & 1u; }

// The set pixel of word m (row y, word column c, padding masked) nearest to the gaze pixel (py, px), as key = d2 * 2^31 + (y * Ws + x):
// the least key over a mask is its nearest set pixel, ties to the first in row-major order.  The candidates are the nearest set bit at
// or left of the gaze column and the nearest at or right of it.  Returns the lesser of `key` and the word's: a pass starts from ~0ull,
// which an empty word leaves as it is.  Sides <= MASK_MAX_SIDE: d2 < 2^29, key < 2^60.
__device__ __forceinline__ unsigned long long mask_near_key(unsigned long long key, unsigned int m, int y, int c, int py, int px, int Ws) {
  if (m == 0u) return key;
  const int pc = px >> 5, pb = px & 31;
  const long long dy = y - py;
  const int x0 = c << 5;
  int xa = -1, xb = -1;
  if (c < pc) xa = x0 + 31 - __clz((int)m);
  else if (c > pc) xb = x0 + __ffs((int)m) - 1;
  else {
    const unsigned int lo = m & (0xffffffffu >> (31 - pb)), hi = m & (0xffffffffu << pb);
    if (lo) xa = x0 + 31 - __clz((int)lo);
    if (hi) xb = x0 + __ffs((int)hi) - 1;
  }
  if (xa >= 0) {
    const long long dx = xa - px;
    const unsigned long long k = ((unsigned long long)(dy * dy + dx * dx) << 31) + (unsigned long long)((long long)y * Ws + xa);
    key = k < key ? k : key;
  }
  if (xb >= 0) {
    const long long dx = xb - px;
    const unsigned long long k = ((unsigned long long)(dy * dy + dx * dx) << 31) + (unsigned long long)((long long)y * Ws + xb);
    key = k < key ? k : key;
  }
  return key;
}
__device__ __forceinline__ unsigned long long mask_key_wave_min(unsigned long long key) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long k = __shfl_xor(key, o, 64);
    key = k < key ? k : key;
  }
  return key;
}

// Word g of bits (words = B * Hs * P of them) is word i of row = b * Hs + y, the columns 32 i .. 32 i + 31.  LPW lanes make one word,
// a workgroup 256 / LPW consecutive ones: LPW = 8, lane l of the eight holds the columns x .. x + 3 = 32 i + 4 l .. (Ws % 4 == 0: the
// quad is inside the row or past its end as a whole); LPW = 32, one lane a column x.  live: the word exists and x < Ws.
struct BitSlot { long g, row; int x; bool live; };
template <int LPW>
__device__ __forceinline__ BitSlot bit_slot(int Ws, int P, long words) {
  BitSlot s;
  s.g = (long)blockIdx.x * (256 / LPW) + threadIdx.x / LPW;
  s.row = s.g / P;
  s.x = 32 * (int)(s.g - s.row * P) + (32 / LPW) * (int)(threadIdx.x % LPW);
  s.live = s.g < words && s.x < Ws;
  return s;
}
// The two stores of word g; every thread of the wave calls them.  Eight lanes a word: nib = the flags of the lane's four columns, or-ed
// over the eight by three shuffles.  One lane a bit: a ballot, two words a wave.  A lane that is not live passes no flag.
__device__ __forceinline__ void store_word_nibbles(unsigned int* __restrict__ bits, long g, long words, unsigned int nib) {
  const int l = threadIdx.x & 7;
  unsigned int wd = nib << (4 * l);
  wd |= __shfl_xor(wd, 1, 64); wd |= __shfl_xor(wd, 2, 64); wd |= __shfl_xor(wd, 4, 64);
  if (l == 0 && g < words) bits[g] = wd;
}
__device__ __forceinline__ void store_word_ballot(unsigned int* __restrict__ bits, long g, long words, bool f) {
  const unsigned long long bal = __ballot(f);
  if ((threadIdx.x & 31) == 0 && g < words) bits[g] = (unsigned int)(bal >> (threadIdx.x & 32));
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
constexpr int MASK_MAX_SIDE = 16384;                   // the most a side where a pass squares distances or packs a pixel index into a key
constexpr long MASK_INT_LIMIT = 2147483647L;           // pixel indices are ints
constexpr long THREADS_MAX = 4294967295L - 255;        // every launch: fewer than 2^32 work-items

// mask_component.hip: the sizes of fs_mask_component and its two passes, for the callers that compose it (unwarp.hip).  ok = launchable
// (positive sizes, sides <= MASK_MAX_SIDE, Hs * Ws < 2^31); scratch in ints; in_lds = the grow pass keeps the reached set in LDS.
struct ComponentPlan {
  int P, pitch, rpr, wpr;
  bool in_lds, ok;
  long scratch;
};
ComponentPlan component_plan(int B, int Hs, int Ws);
int component_launch(const ComponentPlan& p, const unsigned int* bits, const float* focus, unsigned int* out, long long* comp, int* scratch,
                     int B, int Hs, int Ws, int conn, long snap2, hipStream_t stream);

// mask_rle.hip: fs_mask_bits' / fs_mask_rle's sizes, for the callers that compose them (unwarp.hip, gaze_motion.hip).  Scratch of the
// run-length passes, in ints: cnt, last, st, each [B][M], M = Ws * S items an image.
struct RlePlan {
  long P, words;                                       // words per row, of the batch
  long S, M, bpi;                                      // segments per column, items and walk workgroups per image
  long cnt, last, st, total;
  bool bits_ok, ok;                                    // launchable: the bit packing, the run-length passes
};
RlePlan rle_plan(int B, int Hs, int Ws);
int mask_bits_launch(const RlePlan& r, const unsigned char* mask, unsigned int* bits, int Ws, hipStream_t stream);
// zeroed counts, then count, scan, store; the caller has checked its pointers, cap >= 1 and r.ok
int rle_launch(const RlePlan& r, const unsigned int* bits, long long* stats, int* counts, int* s, int B, int Hs, int Ws, int cap,
               hipStream_t stream);
