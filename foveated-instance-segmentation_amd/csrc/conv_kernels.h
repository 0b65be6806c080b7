// Internal interface between conv.hip (C-ABI entry points, kernel selection: plan_conv) and the split-precision kernel families it hands
// a problem to -- forward / bwd-data: conv_halo.hip, conv_wino.hip, conv_wino4.hip, conv_tapset.hip, conv_pointwise.hip, conv_s2fwd.hip,
// conv_s2bwd.hip; bwd-weight: conv_wgrad.hip.  Every forward / bwd-data family takes (mode, FsConvProblem) and runs its weight pack and
// its kernel through fs_pack_then_run (conv_run.h).  Not part of include/fovealseg.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct FsBnSums;
// One forward / bwd-data problem as conv.hip's entry points state it and every family receives it.  NHWC fp32 tensors.  The generic
// kernel of conv.hip takes these bytes by value (as its ConvArgs), so the fields keep their order and the host-only ones stay behind.
struct FsConvProblem {
  const float* src;   // fwd: X (B,Hs,Ws,Cs)      bwd-data: dY
  const float* w;     // [R][S][Cin][Cout]
  const float* bias;  // fwd only, may be null
  float* dst;         // fwd: Y (B,Hd,Wd,Cd)      bwd-data: dX
  int B, Hs, Ws, Cs, Hd, Wd, Cd;
  int R, S, stride, pad, dil;
  int transposed;     // 0 = forward (K = Cin, N = Cout), 1 = bwd-data (K = Cout, N = Cin)
  float drop_scale;   // 1/(1-p)
  uint32_t drop_thresh, drop_key;   // thresh 0 = no dropout
  hipStream_t stream_ = nullptr;    // host only
  float* stats_ = nullptr;          // host only: BN partial-sum slab (forward); bwd-data: where the sums bn_ asks for go
  const FsBnSums* bn_ = nullptr;    // host only: extras fused into the epilogue (FsBnSums below), may be null
  void* ws_ = nullptr;              // host only: caller's scratch for the pre-split weight pack (may be null)
  long ws_bytes_ = 0;
  const unsigned* w_amax_ = nullptr;   // host only: max|w| bits kept by the caller (f16x2 mode), may be null
  int Cin() const { return transposed ? Cd : Cs; }      // the logical weight shape
  int Cout() const { return transposed ? Cs : Cd; }
  long w_elems() const { return (long)R * S * Cs * Cd; }
  size_t src_elems() const { return (size_t)B * Hs * Ws * Cs; }
  size_t dst_elems() const { return (size_t)B * Hd * Wd * Cd; }
};

// ---- conv_halo.hip: halo-tiled 3x3 / stride 1 / pad 1 kernel.  mode: 1 = bf16x3, 2 = f16x2 (conv_split.h) ----------------
// 3x3, stride 1, pad 1, dilation 1, channel counts multiples of 4, K >= 32
bool fs_halo_eligible(int H, int W, int Cs, int Cd, int R, int S, int stride, int pad, int dil);
// bytes of the pre-split weight pack (header included) for K = Cs source channels and N = Cd destination channels
long fs_halo_pack_bytes(int mode, int Cs, int Cd);
// number of pixel tiles (= BatchNorm partial-sum slabs) the kernel uses for a (B,H,W) output
int fs_halo_stats_slabs(int B, int H, int W);
// pack c.w into c.ws_, then run the conv (source and destination have one size).  c.stats_ may be null.
int fs_halo_conv3x3(int mode, const FsConvProblem& c);
// where the f16x2 kernels read max |w| (float bits) of a weight tensor: w_amax when the caller maintains it, else the first
// word of ws, filled here by a memset + atomic-max kernel.
const unsigned* fs_f16_weight_amax(const float* w, long n, void* ws, const unsigned* w_amax, hipStream_t stream, int* err);
// How the calling thread's next conv entry point treats `ws` (fs_conv2d_ws_mode / fs_conv2d_pack, include/fovealseg.h): 0 = pack the
// weights into ws, then run (the default); FS_WS_RUN_ONLY = ws already holds this layer's pack for this shape and precision (the pack
// launch is skipped); FS_WS_PACK_ONLY = run the pack launch and return.  Read by fs_pack_then_run (conv_run.h), which every kernel family
// with a weight pack goes through, by fs_f16_weight_amax and by conv.hip's entry points.
extern thread_local int fs_ws_mode_tls;
#define FS_WS_RUN_ONLY 1
#define FS_WS_PACK_ONLY 2
int fs_weight_amax_segments_impl(const float* arena, const long* offsets, const long* sizes, int nparams, unsigned* out, hipStream_t stream);

// ---- conv_wino.hip: the same problem class with F(2,3) minimal filtering along the row (12 MFMA steps per pixel pair instead of 18).
// Even W >= 4, B*(H+1) < 65536, channel counts multiples of 4, K >= 32 (K >= 128 in f16x2); FS_WINOGRAD=0 switches it off.
// optional epilogue mode of the bwd-data call: BatchNorm-backward column sums of the layer whose output gradient is being written
struct FsBnSums {
  const float* y; const unsigned char* mask; const float* mean; const float* invstd;      // bwd-data: BatchNorm-backward sums of the consumer layer
  const float* add_src; const unsigned char* add_mask;                                    // bwd-data: second gradient joining in the epilogue
  const float* ep_scale; const float* ep_shift; const float* ep_res; int ep_act;          // forward (inference): affine + residual + activation
  // forward of a linear layer that ends a residual branch (1x1 GEMM kernel, round 5): dst = add_src + DropPath(Dropout(conv + bias)) --
  // rows [b * dp_rows, (b + 1) * dp_rows) belong to sample b, kept with the sample hash of fs_residual_droppath (dp_thresh 0: no DropPath)
  float dp_scale; uint32_t dp_thresh, dp_key; int dp_rows;
};
bool fs_wino_eligible(int mode, int B, int H, int W, int Cs, int Cd);
long fs_wino_pack_bytes(int mode, int Cs, int Cd);
int fs_wino_stats_slabs(int mode, int B, int H, int W, int Cs, int Cd);
int fs_wino_conv3x3(int mode, const FsConvProblem& c);      // hands the problems fs_wino_takes_f43 names on to fs_wino4_conv3x3

// ---- conv_wino4.hip (round 5): the same problem class with F(4,3) along the row (18 MFMA steps per four output pixels instead of 24):
// bf16x3 only, W a multiple of 4.  fs_wino_conv3x3 / fs_wino_pack_bytes / fs_wino_stats_slabs route to it where fs_wino4_selected holds.
bool fs_wino_takes_f43(int mode, int B, int H, int W, int Cs, int Cd);      // conv_wino.hip: this problem goes to the F(4,3) kernel
bool fs_wino4_eligible(int mode, int B, int H, int W, int Cs, int Cd);
long fs_wino4_pack_bytes(int mode, int Cs, int Cd);
int fs_wino4_stats_slabs(int B, int H, int W, int Cs, int Cd);
int fs_wino4_conv3x3(int mode, const FsConvProblem& c);

// ---- conv_pointwise.hip: 1x1 / stride 1 / pad 0 as a GEMM with pre-split weights (forward and bwd-data).  mode: 1 = bf16x3, 2 = f16x2 ----
bool fs_pointwise_eligible(int Cs, int Cd, int R, int S, int stride, int pad, int dil);
long fs_pointwise_pack_bytes(int mode, int Cs, int Cd);
// forward of a stride >= filter convolution as one GEMM over gathered rows (K = R*S*Cin; pack bytes = fs_pointwise_pack_bytes(mode, K, Cout))
bool fs_pointwise_gather_eligible(int Cin, int Cout, int R, int S, int stride, int dil);
int fs_pointwise_gather_conv(int mode, const FsConvProblem& c);
// bwd-data of those layers: one GEMM per tap whose rows are scattered to the tap's residue class of dX (the caller zero-fills the classes no
// tap reaches); pack bytes = fs_pointwise_pack_bytes(mode, Cout, Cin)
bool fs_pointwise_scatter_eligible(int Cin, int Cout, int R, int S, int stride, int dil);
int fs_pointwise_scatter_conv(int mode, const FsConvProblem& c);
// M = B*Hd*Wd rows.  c.stats_: [ceil(M/128)][Cd][2] or null.  c.bn_ (may be null): in bwd-data stats_ then receives the BatchNorm-backward
// sums of the layer that produced x, and / or a second gradient joins dst; forward: the residual + DropPath epilogue
int fs_pointwise_conv(int mode, const FsConvProblem& c);
int fs_pointwise_stats_slabs(long M);

// ---- deterministic split-K (include/fovealseg.h fs_set_deterministic) ----------------------------------------------------------
// Every bwd-weight kernel ends by adding its workgroup's partial dW tile to the tiles of the other pixel splits.  By default that is an
// fp32 atomic per element (order = arrival order: results differ in the last bits from run to run).  In deterministic mode each split
// writes its partial tile with plain stores into ITS OWN slab (a full dW image) of the caller's workspace and fs_wgrad_reduce sums the
// slabs in index order.  base == nullptr selects the atomics.
struct FsPart { float* base; long stride; };
__device__ __forceinline__ void fs_wgrad_out(float* dw, const FsPart p, int slab, long idx, float v) {
#ifdef FS_WGRAD_NT
  // kernel A/B builds only (-DFS_WGRAD_NT): the partial tiles leave with non-temporal stores, so that 75 MB of slab lines per launch do
  // not displace the layer's dY / X from L2 between its bwd-weight and its bwd-data (measured in profiles/r05/wgrad_nt_ab.txt)
  if (p.base != nullptr) __builtin_nontemporal_store(v, p.base + (long)slab * p.stride + idx);
#else
  if (p.base != nullptr) p.base[(long)slab * p.stride + idx] = v;
#endif
  else atomicAdd(dw + idx, v);
}
bool fs_deterministic();
// dw[i] = (accumulate ? dw[i] : 0) + part[0][i] + part[1][i] + ... + part[nslab-1][i], in that order
int fs_wgrad_reduce(float* part, int nslab, long n, float* dw, int accumulate, hipStream_t stream);

// ---- conv_wgrad.hip: the bwd-weight plan, and the split-precision weight gradient kernels it launches ----
// any square filter / stride whose tap classes have at most 2 taps per dimension (3x3 s2/s4, 1x1 any stride), plus 3x3 s1
bool fs_wgrad_split_eligible(int Cin, int Cout, int R, int S, int stride, int pad, int dil);
bool fs_wgrad_gather_s2(int Cin, int R, int S, int stride);
bool fs_linear_wgrad_eligible(int mode, long rows, int Cin, int Cout);
// public ids (include/fovealseg.h fs_conv2d_bwd_weight_plan); fs_wgrad_plan has the order in which they are tried
enum FsWgradRoute {
  FS_WG_GENERIC = 0,      // conv_wgrad_kernel<false>  (conv.hip)
  FS_WG_GENERIC_VEC = 1,  // conv_wgrad_kernel<true>   (conv.hip)
  FS_WG_TAPS3 = 2,        // conv_wgrad_taps_kernel<3> (conv.hip)
  FS_WG_TAPS9 = 3,        // conv_wgrad_taps_kernel<9> (conv.hip)
  FS_WG_CLASS33 = 4,      // conv_wgrad_class_kernel<P, 3, 3>, one launch
  FS_WG_WINO = 5,         // conv_wgrad_wino_kernel
  FS_WG_LINEAR = 6,       // linear_wgrad_kernel over plain rows
  FS_WG_GATHER = 7,       // linear_wgrad_kernel over gathered rows, all taps in one launch
  FS_WG_PLANES = 8,       // conv_wgrad_planes_kernel
  FS_WG_CLASSES = 9,      // conv_wgrad_class_kernel<P, 1..2, 1..2>, one launch per tap class
  FS_WG_NROUTES
};
enum FsWgradAccum {
  FS_WG_ATOMIC_ZEROED = 0,  // fp32 atomics into dW after a memset of it
  FS_WG_ATOMIC_ADD = 1,     // fp32 atomics into the caller's accumulating dW
  FS_WG_SLABS_ZEROED = 2,   // memset of `cap` slabs, plain stores, ordered reduce (deterministic mode: a split without pixels writes nothing)
  FS_WG_SLABS_STORED = 3    // plain stores into slabs the launch writes completely, ordered reduce
};
// one launch: patch shape (rows x columns; the transform-domain kernel: rows x pixel pairs; 0 where the kernel has none), split count, and
// patches (rows of the linear kernel, pixels of the fp32 kernels) per split
struct FsWgradStep { int Ph, Pw, nsplit, per_split; };
struct FsWgradPlan {
  bool ok;               // the launch is accepted: a known kernel, and where it writes slabs they fit `cap` and the scratch holds `cap` slabs
  int mode;              // precision mode the plan was made for
  int route, accum;      // FsWgradRoute, FsWgradAccum
  int tile;              // LINEAR / GATHER: tile variant of linear_wgrad_kernel, 1-4
  int prio;              // class kernel: WgArgs::prio
  int nlaunch;           // conv kernel launches (memsets and the reduce not counted)
  FsWgradStep step[9];
  long wgs;              // workgroups of all launches together
  int threads;           // per workgroup
  int slabs;             // slab rows the launches write = slabs the reduce sums; 0 with atomics
  long cap;              // fs_wgrad_slab_cap of the shape: slabs the scratch must hold (and that SLABS_ZEROED zeroes)
};
long fs_wgrad_slab_cap(int mode, int Cin, int Cout, int R, int S, int stride, int pad, int dil);
// slabs of R*S*Cin*Cout floats a caller must provide for this layer: the cap in deterministic mode and for the layers that store, else 0
long fs_wgrad_ws_slabs(int mode, bool det, int Cin, int Cout, int R, int S, int stride, int pad, int dil);
FsWgradPlan fs_wgrad_plan(int mode, bool det, bool accumulate, bool has_ws, long ws_bytes, int B, int H, int W, int Cin, int Ho, int Wo, int Cout,
                          int R, int S, int stride, int pad, int dil);
FsWgradPlan fs_linear_wgrad_plan(bool det, bool accumulate, long rows, int Cin, int Cout);
int fs_wgrad_launch(const FsWgradPlan& p, const float* x, const float* dy, float* dw, float* dbias, FsPart part, float* bpart, int B, int H, int W,
                    int Cin, int Ho, int Wo, int Cout, int R, int S, int stride, int pad, hipStream_t stream);

// ---- conv_s2bwd.hip: bwd-data of a 3x3 / stride 2 / pad 1 convolution, the four output parities in one launch ----
bool fs_s2bwd_eligible(int H, int W, int Cin, int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil);
long fs_s2bwd_pack_bytes(int mode, int Cin, int Cout);
// c.bn_ (may be null): c.stats_[fs_s2bwd_stats_slabs][Cin][2] receives the BatchNorm-backward sums of the layer that produced x, and / or a
// second gradient joins dX
int fs_s2bwd_stats_slabs(int B, int Ho, int Wo);
int fs_s2bwd_conv(int mode, const FsConvProblem& c);

// ---- conv_s2fwd.hip: forward of a 3x3 / stride 2 / pad 1 convolution, the four input parity planes in one LDS refill per chunk ----
bool fs_s2fwd_eligible(int H, int W, int Cin, int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil);
long fs_s2fwd_pack_bytes(int mode, int Cin, int Cout);
int fs_s2fwd_slabs(int B, int Ho, int Wo);          // BatchNorm partial-sum slabs (= pixel tiles) of the stats variant
int fs_s2fwd_conv(int mode, const FsConvProblem& c);

// conv_tapset.hip: general halo-tiled split-precision convolution over a list of tap classes.
//   source row of (loop row oy, class tap tr) = sm*(oy + tr) + cy,  filter row r = rbase + rstep*tr  (columns alike)
struct FsTapClass { int cy, cx, nR, nS, rbase, rstep, sbase, sstep; };
// the problem plus what this family adds: the loop grid (by default the whole destination) and the tap classes
struct FsTapsetProblem : FsConvProblem {
  explicit FsTapsetProblem(const FsConvProblem& c) : FsConvProblem(c), Hq(c.Hd), Wq(c.Wd) {}
  int Hq, Wq, os = 1, oy0 = 0, ox0 = 0, sm = 1;      // destination pixel = (oy*os + oy0, ox*os + ox0), oy < Hq, ox < Wq
  int ncls = 0; FsTapClass cls[9];
};
long fs_tapset_pack_bytes(int mode, int Cs, int Cd, int total_taps);
int fs_tapset_slabs(int B, int Hq, int Wq, int maxR, int maxS);
int fs_tapset_conv(int mode, const FsTapsetProblem& p);      // mode: 1 = bf16x3, 2 = f16x2
void fs_tapset_patch(int Hq, int Wq, int maxR, int maxS, int* Ph, int* Pw);
