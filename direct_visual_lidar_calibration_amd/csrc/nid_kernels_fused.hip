// the fused one-launch evaluation (nid_fused.hpp): instantiations for every camera model, both record types, both stash formats.
// Built with -ffp-contract=off like every other translation unit: the per-point arithmetic is k_spline_hist's / k_spline_grad's.
#include "nid_fused.hpp"
#include "nid_launch_impl.hpp"

namespace nidreg {

size_t fused_lds_bytes_for(const PassArgs& a, int full, int cap) { return fused_lds_bytes(a.B, a.GW, a.cshift, full != 0, a.rec64 ? sizeof(Rec64) : sizeof(Rec32), cap); }

// launches the instantiation `a` and `f` select, or (occ) only asks how many of its workgroups fit on one CU at once
template <typename Rec>
static hipError_t fused_rec(const PassArgs& a, const FusedArgs& f, int* occ) {
  const PoseParams<double> pose = make_pose(a);
  const CamParams<double> cam = make_cam(a.model, a.intr, a.dist);
  GradTail gt = a.gt;
  gt.from_partials = 2;
  return with_model(a.model, hipErrorInvalidValue, [&](auto M) {
    return with_bool(f.full != 0, [&](auto FULL) {
      return launch_chunks(k_spline_fused<M, Rec, FULL>, kThreads, fused_lds_bytes(a.B, a.GW, a.cshift, FULL, sizeof(Rec), f.cap), a, occ, static_cast<const Rec*>(a.pts), a.chunks, a.img,
                           a.pitch, a.W, a.H, pose, cam, a.B, a.GW, a.cshift, a.magic, a.inv_unit, a.hist, gt, a.partials, a.q[0], a.q[1], a.q[2], a.q[3], a.out, a.out_host, a.tag,
                           a.counter, f.barrier, f.barrier_target, f.flags, f.epoch, f.timeout_ticks, f.cap);
    });
  });
}

hipError_t launch_spline_fused(const PassArgs& a, const FusedArgs& f) {
  if (a.nchunks == 0) return hipErrorInvalidValue;
  return a.rec64 ? fused_rec<Rec64>(a, f, nullptr) : fused_rec<Rec32>(a, f, nullptr);
}
int occupancy_spline_fused(const PassArgs& a, const FusedArgs& f) {
  int n = 0;
  return (a.rec64 ? fused_rec<Rec64>(a, f, &n) : fused_rec<Rec32>(a, f, &n)) == hipSuccess ? n : 0;
}

}  // namespace nidreg

#ifdef NID_STAMP
// development aid (tools/fused_stage_times.py, an instrumented build loaded through NIDREG_LIB): the fused kernel's stage stamps
extern "C" int nidreg_debug_fused_stage_stamps(unsigned long long* out, int words) {
  return int(hipMemcpyFromSymbol(out, HIP_SYMBOL(nidreg::g_stage), size_t(words) * sizeof(unsigned long long)));
}
#endif
