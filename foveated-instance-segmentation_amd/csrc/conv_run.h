// Host-side steps the split-precision forward / bwd-data families share between "plan_conv chose this family" and "its kernel is in the
// stream" (conv_halo.hip, conv_wino.hip, conv_wino4.hip, conv_tapset.hip, conv_pointwise.hip, conv_s2fwd.hip, conv_s2bwd.hip).
#pragma once
#include "conv_kernels.h"
#include "conv_split.h"

// ---- the ws-mode protocol (fs_ws_mode_tls, conv_kernels.h), once ---------------------------------------------------------------
// pack(P{}, ew) launches the family's weight pack into c.ws_; run(P{}, ew) launches its conv kernel and returns FS_OK, or an error
// it met before the launch.  ew = where the f16x2 kernels read max|w| bits (null in bf16x3).  Both launches are checked here.
template <class P, class Pack, class Run>
int fs_pack_then_run_as(const FsConvProblem& c, Pack&& pack, Run&& run) {
  int e = FS_OK;
  const unsigned* ew = P::SCALED ? fs_f16_weight_amax(c.w, c.w_elems(), c.ws_, c.w_amax_, c.stream_, &e) : nullptr;
  if (e != FS_OK) return e;
  if (fs_ws_mode_tls != FS_WS_RUN_ONLY) {
    pack(P{}, ew);
    FS_LAUNCH_CHECK();
  }
  if (fs_ws_mode_tls == FS_WS_PACK_ONLY) return FS_OK;
  e = run(P{}, ew);
  if (e != FS_OK) return e;
  FS_LAUNCH_CHECK();
  return FS_OK;
}
// mode: 1 = bf16x3, 2 = f16x2
template <class Pack, class Run>
int fs_pack_then_run(int mode, const FsConvProblem& c, Pack&& pack, Run&& run) {
  return mode == 2 ? fs_pack_then_run_as<fs_split::PrecF16>(c, pack, run) : fs_pack_then_run_as<fs_split::PrecX3>(c, pack, run);
}
// grid of a pack kernel with one thread per row: total rows / 256
static inline dim3 fs_pack_grid(long total) { return dim3((unsigned)((total + 255) / 256)); }

// ---- kernel-argument fills ---------------------------------------------------------------------------------------------------------
// The kernels address tensors and the pack through raw buffer resources with 32-bit byte offsets: false when one of the three does not
// fit, else the *_bytes fields of the kernel arguments are set.
static inline bool fs_sizes32(long pack_bytes, size_t src_elems, size_t dst_elems, unsigned& src_bytes, unsigned& dst_bytes, unsigned& ws_bytes) {
  if (pack_bytes >= 2147483647L || src_elems * 4 >= 4294967000UL || dst_elems * 4 >= 4294967000UL) return false;
  src_bytes = (unsigned)(src_elems * 4);
  dst_bytes = (unsigned)(dst_elems * 4);
  ws_bytes = (unsigned)pack_bytes;
  return true;
}
// bwd-data extras of FsBnSums -> the kernel arguments of a family that fuses them (bn may be null: all off)
template <class A>
void fs_fill_bwd_extras(A& a, const FsBnSums* bn) {
  a.bn_y = bn ? bn->y : nullptr; a.bn_mask = bn ? bn->mask : nullptr; a.bn_mean = bn ? bn->mean : nullptr; a.bn_invstd = bn ? bn->invstd : nullptr;
  a.add_src = bn ? bn->add_src : nullptr; a.add_mask = bn ? bn->add_mask : nullptr;
}
// ... and the forward (inference) affine + residual + activation epilogue
template <class A>
void fs_fill_fwd_epilogue(A& a, const FsBnSums* bn) {
  a.ep_scale = bn ? bn->ep_scale : nullptr; a.ep_shift = bn ? bn->ep_shift : nullptr; a.ep_res = bn ? bn->ep_res : nullptr; a.ep_act = bn ? bn->ep_act : 0;
}
