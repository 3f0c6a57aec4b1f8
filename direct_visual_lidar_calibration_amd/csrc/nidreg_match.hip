// nidreg_match.hip -- C ABI of find_matches (include/nidreg.h: nidreg_features_detect, nidreg_features_match): FAST/BRIEF keypoints
// over a 6/5 pyramid and mutual-best Hamming matching on the device (kernels: nid_match_kernels.hpp).  A classical stand-in for the
// reference's scripts/find_matches_superglue.py, of which only the command line and the JSON keys are kept (find_matches.py).
#include "nid_match_kernels.hpp"
#include "nid_host.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

using namespace nidreg;

namespace {

dim3 tiles(int w, int h) { return dim3(blocks_for(w, kFeatTileW), blocks_for(h, kFeatTileH)); }

}  // namespace

extern "C" {

int nidreg_features_detect(int device_id, const uint8_t* image, int width, int height, int64_t row_stride, const uint8_t* mask, int64_t mask_row_stride, int levels,
                           int fast_threshold, int nms_radius, int fill_passes, int max_keypoints, int32_t* kpts_out, uint32_t* desc_out, int32_t* count_out) {
  const char* const who = "nidreg_features_detect";
  if (!image || !kpts_out || !desc_out || !count_out) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null argument");
  if (width <= 0 || height <= 0 || width > kFeatMaxDim || height > kFeatMaxDim)
    return fail(NIDREG_ERR_INVALID, std::string(who) + ": width and height must lie in [1, " + std::to_string(kFeatMaxDim) + "]");
  if (row_stride < width || (mask && mask_row_stride < width)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": a row stride below the width");
  if (levels < 1 || levels > kFeatMaxLevels) return fail(NIDREG_ERR_INVALID, std::string(who) + ": levels must lie in [1, " + std::to_string(kFeatMaxLevels) + "]");
  if (fast_threshold < 1 || fast_threshold > 255 || nms_radius < 0 || nms_radius > kFeatMaxRadius || fill_passes < 0 || fill_passes > 64)
    return fail(NIDREG_ERR_INVALID, std::string(who) + ": fast_threshold in [1, 255], nms_radius in [0, 16], fill_passes in [0, 64] expected");
  if (max_keypoints == 0 || max_keypoints < -1 || max_keypoints > NIDREG_FEATURES_CAPACITY)
    return fail(NIDREG_ERR_INVALID, std::string(who) + ": max_keypoints must be -1 or in [1, " + std::to_string(NIDREG_FEATURES_CAPACITY) + "]");
  const int cap = max_keypoints < 0 ? NIDREG_FEATURES_CAPACITY : max_keypoints;

  // the levels that can hold a keypoint: both sides > 2 x border.  The rest produce none and are not built.
  FeatLevels lv;
  std::memset(&lv, 0, sizeof(lv));
  lv.W0 = width, lv.H0 = height;
  int nl = 0;
  int64_t total = 0;
  std::vector<int64_t> off;
  for (int l = 0, w = width, h = height; l < levels && w > 2 * kFeatBorder && h > 2 * kFeatBorder; l++, w = 5 * w / 6, h = 5 * h / 6) {
    lv.w[l] = w, lv.h[l] = h;
    lv.num[l] = l ? lv.num[l - 1] * 6 : 1, lv.den[l] = l ? lv.den[l - 1] * 5 : 2;
    off.push_back(total);
    total += int64_t(w) * h;
    nl = l + 1;
  }
  *count_out = 0;
  if (nl == 0) return NIDREG_OK;  // nothing to launch
  if (total > 2147483647LL) return fail(NIDREG_ERR_INVALID, std::string(who) + ": more than 2^31 - 1 pyramid pixels");
  if (const int rc = use_device(who, device_id)) return rc;

  const size_t n0 = size_t(width) * size_t(height), nt = size_t(total);
  // levels (unsmoothed) and their smoothed copies, level offsets shared; the score map of one level at a time; two sort buffers
  DeviceBuf d_pyr, d_smooth, d_score, d_keys, d_keys2, d_tmp, d_mask, d_fill, d_count, d_kpts, d_desc;
  HIP_TRY(d_pyr.alloc(nt));
  HIP_TRY(d_smooth.alloc(nt));
  HIP_TRY(d_score.alloc(n0));
  HIP_TRY(d_keys.alloc(nt * sizeof(match_u64)));
  HIP_TRY(d_keys2.alloc(nt * sizeof(match_u64)));
  HIP_TRY(d_count.alloc(sizeof(int)));
  HIP_TRY(hipMemcpy2D(d_pyr.as<void>(), size_t(width), image, size_t(row_stride), size_t(width), size_t(height), hipMemcpyHostToDevice));
  uint8_t* const pyr = d_pyr.as<uint8_t>();
  uint8_t* const smooth = d_smooth.as<uint8_t>();
  if (mask) {
    // [0] the caller's mask (kept: the validity of a keypoint), then two image / mask pairs for the ping-pong of the fill passes
    HIP_TRY(d_mask.alloc(n0));
    HIP_TRY(hipMemcpy2D(d_mask.as<void>(), size_t(width), mask, size_t(mask_row_stride), size_t(width), size_t(height), hipMemcpyHostToDevice));
    if (fill_passes > 0) {
      HIP_TRY(d_fill.alloc(3 * n0));
      uint8_t* const f = d_fill.as<uint8_t>();
      uint8_t *img_a = pyr, *msk_a = f, *img_b = f + n0, *msk_b = f + 2 * n0;
      HIP_TRY(hipMemcpyAsync(msk_a, d_mask.as<void>(), n0, hipMemcpyDeviceToDevice, nullptr));
      for (int p = 0; p < fill_passes; p++) {
        HIP_TRY(launch(k_fill_pass, tiles(width, height), kFeatThreads, 0, nullptr, img_a, msk_a, img_b, msk_b, width, height));
        std::swap(img_a, img_b), std::swap(msk_a, msk_b);
      }
      if (img_a != pyr) HIP_TRY(hipMemcpyAsync(pyr, img_a, n0, hipMemcpyDeviceToDevice, nullptr));
    }
  }
  for (int l = 0; l < nl; l++) {
    uint8_t* const cur = pyr + off[size_t(l)];
    const int w = lv.w[l], h = lv.h[l];
    if (l > 0) HIP_TRY(launch(k_pyr_down, tiles(w, h), kFeatThreads, 0, nullptr, pyr + off[size_t(l - 1)], lv.w[l - 1], lv.h[l - 1], cur, w, h));
    lv.smooth[l] = smooth + off[size_t(l)];
    HIP_TRY(launch(k_smooth, tiles(w, h), kFeatThreads, 0, nullptr, cur, w, h, smooth + off[size_t(l)]));
    HIP_TRY(launch(k_fast_score, tiles(w, h), kFeatThreads, 0, nullptr, cur, w, h, d_score.as<uint8_t>()));
    HIP_TRY(launch(k_nms_keys, tiles(w, h), kFeatThreads, 0, nullptr, d_score.as<uint8_t>(), w, h, l, nms_radius, fast_threshold, d_mask.as<uint8_t>(), width, height, lv.num[l], lv.den[l],
                   d_keys.as<match_u64>() + off[size_t(l)]));
  }
  // the order of the keypoints is the order of their keys (48 significant bits; kFeatNoKey's low 48 bits are all ones: last)
  size_t tmp_bytes = 0;
  HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp_bytes, d_keys.as<match_u64>(), d_keys2.as<match_u64>(), nt, 0, 48, hipStream_t(nullptr)));
  HIP_TRY(d_tmp.alloc(std::max<size_t>(tmp_bytes, 16)));
  HIP_TRY(rocprim::radix_sort_keys(d_tmp.as<void>(), tmp_bytes, d_keys.as<match_u64>(), d_keys2.as<match_u64>(), nt, 0, 48, hipStream_t(nullptr)));
  HIP_TRY(hipMemsetAsync(d_count.as<void>(), 0, sizeof(int), nullptr));
  HIP_TRY(launch(k_count_keys, blocks_for(total, kFeatThreads), kFeatThreads, 0, nullptr, d_keys2.as<match_u64>(), int(total), d_count.as<int>()));
  int found = 0;
  HIP_TRY(hipMemcpy(&found, d_count.as<void>(), sizeof(int), hipMemcpyDeviceToHost));  // (synchronises the null stream)
  const int n = std::min(found, cap);
  if (n > 0) {
    HIP_TRY(d_kpts.alloc(size_t(n) * 4 * sizeof(int32_t)));
    HIP_TRY(d_desc.alloc(size_t(n) * 8 * sizeof(uint32_t)));
    HIP_TRY(launch(k_describe, unsigned(n), kBriefPairs, 0, nullptr, d_keys2.as<match_u64>(), lv, d_kpts.as<int32_t>(), d_desc.as<uint32_t>()));
    HIP_TRY(hipMemcpy(kpts_out, d_kpts.as<void>(), size_t(n) * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(desc_out, d_desc.as<void>(), size_t(n) * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  *count_out = n;
  return NIDREG_OK;
}

int nidreg_features_match(int device_id, const uint32_t* desc0, int n0, const uint32_t* desc1, int n1, int max_distance, int ratio_num, int ratio_den, int32_t* match01_out,
                          int32_t* dist_out, int32_t* second_out) {
  const char* const who = "nidreg_features_match";
  if (n0 < 0 || n1 < 0 || (n0 > 0 && (!desc0 || !match01_out || !dist_out)) || (n1 > 0 && !desc1)) return fail(NIDREG_ERR_INVALID, std::string(who) + ": null argument or negative count");
  if (ratio_den <= 0 || ratio_num < 0 || max_distance < 0) return fail(NIDREG_ERR_INVALID, std::string(who) + ": ratio_den > 0, ratio_num >= 0 and max_distance >= 0 expected");
  if (n0 == 0) return NIDREG_OK;
  if (n1 == 0) {  // no column: no match, both distances the sentinel; nothing to launch
    for (int i = 0; i < n0; i++) {
      match01_out[i] = -1, dist_out[i] = kHammingNone;
      if (second_out) second_out[i] = kHammingNone;
    }
    return NIDREG_OK;
  }
  if (const int rc = use_device(who, device_id)) return rc;
  const size_t s0 = size_t(n0), s1 = size_t(n1);
  // one result block: rows' best / distance / second / match, then the columns' best / distance / second
  DeviceBuf d_desc, d_res;
  HIP_TRY(d_desc.alloc((s0 + s1) * 32));
  HIP_TRY(d_res.alloc((4 * s0 + 3 * s1) * sizeof(int32_t)));
  uint32_t* const d0 = d_desc.as<uint32_t>();
  uint32_t* const d1 = d0 + 8 * s0;
  HIP_TRY(hipMemcpy(d0, desc0, s0 * 32, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d1, desc1, s1 * 32, hipMemcpyHostToDevice));
  int32_t* const r = d_res.as<int32_t>();
  int32_t *best01 = r, *dist01 = r + s0, *sec01 = r + 2 * s0, *match = r + 3 * s0, *best10 = r + 4 * s0, *dist10 = best10 + s1, *sec10 = best10 + 2 * s1;
  HIP_TRY(launch(k_hamming_best, blocks_for(n0, kMatchThreads), kMatchThreads, 0, nullptr, d0, n0, d1, n1, best01, dist01, sec01));
  HIP_TRY(launch(k_hamming_best, blocks_for(n1, kMatchThreads), kMatchThreads, 0, nullptr, d1, n1, d0, n0, best10, dist10, sec10));
  HIP_TRY(launch(k_mutual, blocks_for(n0, kFeatThreads), kFeatThreads, 0, nullptr, n0, best01, dist01, sec01, best10, max_distance, ratio_num, ratio_den, match));
  std::vector<int32_t> out(4 * s0);
  HIP_TRY(hipMemcpy(out.data(), r, 4 * s0 * sizeof(int32_t), hipMemcpyDeviceToHost));  // (synchronises the null stream)
  std::memcpy(dist_out, out.data() + s0, s0 * sizeof(int32_t));
  if (second_out) std::memcpy(second_out, out.data() + 2 * s0, s0 * sizeof(int32_t));
  std::memcpy(match01_out, out.data() + 3 * s0, s0 * sizeof(int32_t));
  return NIDREG_OK;
}

}  // extern "C"
