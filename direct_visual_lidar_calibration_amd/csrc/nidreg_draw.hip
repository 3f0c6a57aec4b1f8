// nidreg_draw.hip -- C ABI of the match pictures (include/nidreg.h: nidreg_draw): lines, rings and discs over one gray image or two
// side by side, on the device (kernels: nid_draw_kernels.hpp).  Stateless, like nidreg_generate_lidar_image: upload, three
// operations on the null stream (owner words zeroed, k_draw_prims, k_draw_compose), copy back.
#include "nid_draw_kernels.hpp"
#include "nid_host.hpp"

using namespace nidreg;

extern "C" {

int nidreg_draw(int device_id, const uint8_t* left_gray, int left_w, int left_h, int64_t left_row_stride, const uint8_t* right_gray, int right_w, int right_h, int64_t right_row_stride,
                int64_t num_prims, const int32_t* prims, uint8_t* out_rgb) {
  const std::string who = "nidreg_draw";
  // every refusal comes before the device is touched, and nothing is written
  if (!left_gray || !out_rgb) return fail(NIDREG_ERR_INVALID, who + ": null left_gray or out_rgb");
  if (num_prims < 0 || num_prims > kDrawMaxPrims) return fail(NIDREG_ERR_INVALID, who + ": num_prims must lie in [0, " + std::to_string(kDrawMaxPrims) + "]");
  if (num_prims > 0 && !prims) return fail(NIDREG_ERR_INVALID, who + ": null prims with num_prims > 0");
  const auto dim_ok = [](int v) { return v >= 1 && v <= kDrawMaxDim; };
  if (!dim_ok(left_w) || !dim_ok(left_h) || (right_gray && (!dim_ok(right_w) || !dim_ok(right_h))))
    return fail(NIDREG_ERR_INVALID, who + ": width and height must lie in [1, " + std::to_string(kDrawMaxDim) + "]");
  if (left_row_stride < left_w || (right_gray && right_row_stride < right_w)) return fail(NIDREG_ERR_INVALID, who + ": a row stride below the width");
  const auto coord_ok = [](int32_t v) { return v >= kDrawCoordMin && v <= kDrawCoordMax; };
  for (int64_t i = 0; i < num_prims; i++) {
    const int32_t* r = prims + i * kDrawWords;
    const std::string at = who + ": primitive " + std::to_string(i) + ": ";
    if (r[0] != kDrawLine && r[0] != kDrawRing && r[0] != kDrawDisc) return fail(NIDREG_ERR_INVALID, at + "unknown kind " + std::to_string(r[0]));
    if (!coord_ok(r[1]) || !coord_ok(r[2]) || (r[0] == kDrawLine && (!coord_ok(r[3]) || !coord_ok(r[4]))))
      return fail(NIDREG_ERR_INVALID, at + "a coordinate outside [" + std::to_string(kDrawCoordMin) + ", " + std::to_string(kDrawCoordMax) + "]");
    if (r[0] != kDrawLine && (r[3] < 0 || r[3] > kDrawMaxRadius)) return fail(NIDREG_ERR_INVALID, at + "radius must lie in [0, " + std::to_string(kDrawMaxRadius) + "]");
    if (r[5] < 0 || r[5] > 0xFFFFFF) return fail(NIDREG_ERR_INVALID, at + "rgb above 0xFFFFFF");
  }
  if (const int rc = use_device(who.c_str(), device_id)) return rc;

  const int cw = right_gray ? 2 * left_w : left_w;
  const size_t npix = size_t(cw) * size_t(left_h);
  DeviceBuf d_left, d_right, d_prims, d_owner, d_out;
  HIP_TRY(d_left.alloc(size_t(left_w) * size_t(left_h)));
  HIP_TRY(hipMemcpy2D(d_left.as<void>(), size_t(left_w), left_gray, size_t(left_row_stride), size_t(left_w), size_t(left_h), hipMemcpyHostToDevice));
  if (right_gray) {
    HIP_TRY(d_right.alloc(size_t(right_w) * size_t(right_h)));
    HIP_TRY(hipMemcpy2D(d_right.as<void>(), size_t(right_w), right_gray, size_t(right_row_stride), size_t(right_w), size_t(right_h), hipMemcpyHostToDevice));
  }
  HIP_TRY(d_owner.alloc(npix * sizeof(uint32_t)));
  HIP_TRY(d_out.alloc(npix * 3));
  HIP_TRY(hipMemsetAsync(d_owner.as<void>(), 0, npix * sizeof(uint32_t), nullptr));
  if (num_prims > 0) {
    const size_t bytes = size_t(num_prims) * kDrawWords * sizeof(int32_t);
    HIP_TRY(d_prims.alloc(bytes));
    HIP_TRY(hipMemcpy(d_prims.as<void>(), prims, bytes, hipMemcpyHostToDevice));
    HIP_TRY(launch(k_draw_prims, unsigned(num_prims), kDrawWave, 0, nullptr, d_prims.as<int32_t>(), cw, left_h, d_owner.as<uint32_t>()));
  }
  HIP_TRY(launch(k_draw_compose, blocks_for(npix, kDrawThreads), kDrawThreads, 0, nullptr, d_left.as<uint8_t>(), left_w, left_h, d_right.as<uint8_t>(), right_w, right_h, cw,
                 d_owner.as<uint32_t>(), d_prims.as<int32_t>(), d_out.as<uint8_t>()));
  HIP_TRY(hipMemcpy(out_rgb, d_out.as<void>(), npix * 3, hipMemcpyDeviceToHost));  // (synchronises the null stream)
  return NIDREG_OK;
}

}  // extern "C"
