// nid_las_kernels.hpp -- ASPRS LAS point records -> VoxFrameF64 (nidreg_integrator_insert_las): the records of a .las map, as they
// lie in the file, to the double frame the voxel integrator's passes read (nid_voxel_kernels.hpp).  Written from the public LAS
// 1.0 - 1.4 specification; UNPINNED against laspy / PDAL and real files (tests/las_oracle.py is a numpy restatement).
//
// A record is `step` bytes (the format's base length plus any extra bytes; 20 .. 65535) and aligns nothing -- a format-2 record is
// 26 bytes --, so every field is put together from single bytes (little-endian), like k_vox_decode_cloud2's, and the tiling is
// that kernel's: one workgroup per tile of kVoxThreads consecutive records, the tile's byte span (widened to 16-byte boundaries;
// the raw buffer is 16-byte aligned and padded to a multiple of 16) copied into LDS with 16-byte loads when step <= kVoxStageStep,
// read from global memory directly otherwise.
//   coordinate   X, Y, Z are int32 at bytes 0, 4, 8.  (double(X) * scale + offset) - origin: three separately rounded fp64
//                operations in that order (the TU is built with -ffp-contract=off; no fma is written).  The first two are the
//                format's definition of the coordinate; the third recentres a georeferenced map BEFORE anything is narrowed to
//                float32 (VoxSlot::rec).
//   intensity    the u16 at byte 12, or with `rgb` 77 R + 150 G + 29 B of the three u16 channels: an exact integer < 2^24.
//   filters      class: low 5 bits of byte 15 (formats 0 - 5) or byte 16 (formats 6 - 10); withheld: bit 7 (0 - 5) or bit 2 (6 - 10)
//                of byte 15.  A point whose class is in the 256-bit mask, or that is withheld when withheld points are dropped, is
//                written with NaN coordinates: k_vox_check then counts it as skipped and it still takes its sequence number,
//                exactly as a non-finite PointCloud2 point does.  Nothing else can be non-finite (the host refuses a non-finite
//                scale, offset or origin), so the skipped count is the filtered count.  No counters and no atomics here.
// The byte offsets and bit masks are derived from the format number on the host and passed by value.
#pragma once
#include "nid_voxel_kernels.hpp"

namespace nidreg {

struct VoxLas {
  const unsigned char* raw;  // n records of `step` bytes
  long long n;
  int step;
  int o_rgb;                 // byte offset of the u16 red channel (green, blue follow); < 0: the intensity is the u16 at byte 12
  int o_class;               // byte that holds the class
  unsigned class_bits;       // 0x1f or 0xff: the bits of that byte that are the class
  unsigned withheld_drop;    // the withheld bit of byte 15, or 0 when withheld points are kept
  double sx, sy, sz, ox, oy, oz, gx, gy, gz;  // scale, offset, origin
};

__device__ inline double las_coord(const unsigned char* p, double scale, double offset, double origin) {
  const int v = int(unsigned(vox_le<4>(p)));  // two's complement: the sign survives the byte assembly
  const double scaled = double(v) * scale;
  const double placed = scaled + offset;
  return placed - origin;
}

template <bool Staged>
__global__ __launch_bounds__(kVoxThreads) void k_vox_decode_las(VoxLas c, vox_u64 m0, vox_u64 m1, vox_u64 m2, vox_u64 m3, double4* pts, double* inten) {
  __shared__ uint4 stage[Staged ? kVoxStageVecs : 1];
  const long long tiles = (c.n + kVoxThreads - 1) / kVoxThreads;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {  // (uniform per workgroup: the barriers below are met by all lanes)
    const long long i0 = t * kVoxThreads, i = i0 + threadIdx.x;
    const unsigned char* rec;
    if constexpr (Staged) {
      const long long i1 = i0 + kVoxThreads < c.n ? i0 + kVoxThreads : c.n;
      const long long b0 = i0 * c.step, a0 = b0 & ~15LL;
      const int vecs = int((i1 * c.step - a0 + 15) >> 4);  // <= kVoxStageVecs: step <= kVoxStageStep
      const uint4* src = reinterpret_cast<const uint4*>(c.raw + a0);
      __syncthreads();  // the previous tile has been read
      for (int v = threadIdx.x; v < vecs; v += kVoxThreads) stage[v] = src[v];
      __syncthreads();
      rec = reinterpret_cast<const unsigned char*>(stage) + (b0 - a0) + (long long)threadIdx.x * c.step;
    } else {
      rec = c.raw + i * c.step;
    }
    if (i < c.n) {
      const unsigned cls = unsigned(rec[c.o_class]) & c.class_bits;
      const vox_u64 word = cls < 64 ? m0 : cls < 128 ? m1 : cls < 192 ? m2 : m3;
      const bool drop = ((word >> (cls & 63)) & 1ULL) != 0 || (unsigned(rec[15]) & c.withheld_drop) != 0;
      double w;
      if (c.o_rgb >= 0) {
        const unsigned r = unsigned(vox_le<2>(rec + c.o_rgb)), g = unsigned(vox_le<2>(rec + c.o_rgb + 2)), b = unsigned(vox_le<2>(rec + c.o_rgb + 4));
        w = double(77u * r + 150u * g + 29u * b);
      } else {
        w = double(unsigned(vox_le<2>(rec + 12)));
      }
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
      const double x = las_coord(rec, c.sx, c.ox, c.gx), y = las_coord(rec + 4, c.sy, c.oy, c.gy), z = las_coord(rec + 8, c.sz, c.oz, c.gz);
      pts[i] = drop ? make_double4(nan, nan, nan, 0.0) : make_double4(x, y, z, 0.0);
      inten[i] = w;
    }
  }
}

}  // namespace nidreg
