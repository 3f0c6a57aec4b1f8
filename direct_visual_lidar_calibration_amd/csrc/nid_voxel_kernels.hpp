// nid_voxel_kernels.hpp -- the voxel integrator of vlcal::StaticPointCloudIntegrator
// (src/vlcal/preprocess/static_point_cloud_integrator.cpp:25-62) as a device-resident hash table.
//
// The reference walks the points in order and does `voxelgrid[floor(p / res)] = (x, y, z, intensity)`: one entry per occupied
// voxel, the LAST point inserted into it.  Here every point carries a sequence number -- the number of points offered to the
// integrator before it, over the integrator's lifetime -- and the entry of a voxel is the point with the LARGEST sequence
// number, which no longer depends on the order the GPU visits the points in:
//   k_vox_check    one pass over the frame before anything is inserted: counts the points with a non-finite coordinate, the
//                  points whose voxel does not fit the packed key, and the points past the distance gate.
//   k_vox_claim    per point: the voxel (true division and floor in double: -0.1 at res 0.25 is voxel -1), its slot by linear
//                  probing -- ONE 64-bit compare-and-swap on the packed key claims an empty slot; identity is the full key,
//                  never its hash -- and a 64-bit atomicMax of (sequence number + 1) into the slot.  The slot found is kept
//                  per point for the next pass.
//   k_vox_payload  after the maxima have settled (the next launch): the one point whose sequence number the slot holds
//                  writes its float32 record (x, y, z, intensity; `cast<float>()`, :55-56) into the slot.  Plain stores, no
//                  float atomics anywhere: the table's contents are a function of the input alone.
//   k_vox_decode_cloud2  nidreg_integrator_insert_cloud2 only: the raw sensor_msgs/PointCloud2 records, as they lie in the message,
//                  to the double frame (VoxFrameF64) the three passes above read.
//   k_vox_rehash   growth: every occupied slot of the old table moves, payload and all, into a table twice (or more) as large.
//   k_vox_compact / k_vox_gather   nidreg_integrator_get: (sequence number, slot) of the occupied slots, radix-sorted by the
//                  host side, then the records in that order.
// PACKED KEY (the one narrowing against the reference, whose key is three `int`s): 21 bits per axis, voxel index + 2^20, so a
// voxel index must lie in [-2^20, 2^20) on every axis -- +-2.1 km at the reference's 2 mm map resolution.  Stored + 1: an all-zero
// slot is empty, so a fresh table is one memset.
// ORDER of nidreg_integrator_get: ascending sequence number of the voxels' winners (the reference's is std::unordered_map
// iteration order, i.e. unspecified); deterministic and identical from run to run.
// (The kernels that are not templates are `static`: nidreg_odom.hip includes this header too.)
// At map resolution nearly every point claims a slot of its own: the atomics have distinct destinations, there is nothing to
// aggregate on chip first, and the kernels are bound by the latency of random 32-byte accesses (slot = key, sequence number and
// payload in ONE 32-byte sector).  Compiled with -ffp-contract=off: +, *, /, sqrt, floor as the host's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nidreg {

typedef unsigned long long vox_u64;

constexpr int kVoxThreads = 256;
constexpr int kVoxMaxBlocks = 2048;              // 256 CUs x 8 workgroups; longer inputs are grid-strided
constexpr long long kVoxAxisLimit = 1LL << 20;   // voxel index in [-kVoxAxisLimit, kVoxAxisLimit) on every axis
constexpr unsigned kVoxNoSlot = 0xffffffffu;     // k_vox_claim's per-point slot of a point behind the distance gate

struct alignas(32) VoxSlot {
  vox_u64 key;  // packed voxel + 1; 0 = empty
  vox_u64 seq;  // largest (sequence number + 1) offered to this voxel
  float4 rec;   // x y z intensity of the point that holds `seq`
};

// the frame as uploaded: 16-byte float records (the stored PLY record), or 32-byte double points + 8-byte double intensities
struct VoxFrameF32 {
  const float4* recs;
  __device__ void load(long long i, double& x, double& y, double& z, double& w) const {
    const float4 r = recs[i];
    x = double(r.x), y = double(r.y), z = double(r.z), w = double(r.w);  // exact
  }
};
struct VoxFrameF64 {
  const double4* pts;  // x y z (w unused)
  const double* inten;
  __device__ void load(long long i, double& x, double& y, double& z, double& w) const {
    const double4 p = pts[i];
    x = p.x, y = p.y, z = p.z, w = inten[i];
  }
};

enum { kVoxSkip = 0, kVoxOk = 1, kVoxNonFinite = 2, kVoxRange = 3 };

// static_point_cloud_integrator.cpp:30-35 for one point.  The norm is Eigen's unrolled reduction of three terms,
// x^2 + (y^2 + z^2); an overflowing square makes the norm infinite, the point passes the gate and is then out of range.
__device__ inline int vox_classify(double x, double y, double z, double res, double min_distance, vox_u64& key) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return kVoxNonFinite;
  if (sqrt(x * x + (y * y + z * z)) < min_distance) return kVoxSkip;
  const double fx = floor(x / res), fy = floor(y / res), fz = floor(z / res);
  const double L = double(kVoxAxisLimit);
  if (!(fx >= -L && fx < L && fy >= -L && fy < L && fz >= -L && fz < L)) return kVoxRange;
  key = (vox_u64((long long)fx + kVoxAxisLimit) | (vox_u64((long long)fy + kVoxAxisLimit) << 21) | (vox_u64((long long)fz + kVoxAxisLimit) << 42)) + 1ULL;
  return kVoxOk;
}

__device__ inline vox_u64 vox_mix(vox_u64 z) {  // splitmix64's finaliser: where probing starts, nothing more
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

// the slot of `key`, claiming an empty one if the key is not in the table yet (the caller keeps the load factor <= 1/2, so the
// probe ends); *claimed = this call took an empty slot
__device__ inline unsigned vox_find_or_claim(VoxSlot* slots, unsigned mask, vox_u64 key, bool* claimed) {
  unsigned h = unsigned(vox_mix(key)) & mask;
  *claimed = false;
  for (;;) {
    vox_u64 old = __atomic_load_n(&slots[h].key, __ATOMIC_RELAXED);
    if (old == 0) {
      old = atomicCAS(&slots[h].key, 0ULL, key);
      if (old == 0) {
        *claimed = true;
        return h;
      }
    }
    if (old == key) return h;
    h = (h + 1) & mask;
  }
}

__device__ inline vox_u64 vox_wave_sum(vox_u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// counters[1] += points with a non-finite coordinate, [2] += points whose voxel does not fit the key, [3] += points past the gate
template <typename Frame>
__global__ __launch_bounds__(kVoxThreads) void k_vox_check(Frame frame, long long n, double res, double min_distance, vox_u64* counters) {
  vox_u64 bad_nf = 0, bad_range = 0, ok = 0;
  const long long stride = (long long)gridDim.x * kVoxThreads;
  for (long long i = (long long)blockIdx.x * kVoxThreads + threadIdx.x; i < n; i += stride) {
    double x, y, z, w;
    frame.load(i, x, y, z, w);
    vox_u64 key;
    const int st = vox_classify(x, y, z, res, min_distance, key);
    bad_nf += st == kVoxNonFinite, bad_range += st == kVoxRange, ok += st == kVoxOk;
  }
  bad_nf = vox_wave_sum(bad_nf), bad_range = vox_wave_sum(bad_range), ok = vox_wave_sum(ok);
  if ((threadIdx.x & 63) == 0) {
    if (bad_nf) atomicAdd(&counters[1], bad_nf);
    if (bad_range) atomicAdd(&counters[2], bad_range);
    if (ok) atomicAdd(&counters[3], ok);
  }
}

// points [i0, i0 + n) of the frame; point i0 + k has sequence number seq0 + k.  slot_of[k] = its slot or kVoxNoSlot;
// counters[0] += slots claimed.
template <typename Frame>
__global__ __launch_bounds__(kVoxThreads) void k_vox_claim(Frame frame, long long i0, long long n, vox_u64 seq0, double res, double min_distance, VoxSlot* slots, unsigned mask,
                                                           unsigned* slot_of, vox_u64* counters) {
  const long long stride = (long long)gridDim.x * kVoxThreads;
  for (long long k = (long long)blockIdx.x * kVoxThreads + threadIdx.x; k < n; k += stride) {
    double x, y, z, w;
    frame.load(i0 + k, x, y, z, w);
    vox_u64 key;
    unsigned h = kVoxNoSlot;
    if (vox_classify(x, y, z, res, min_distance, key) == kVoxOk) {  // (k_vox_check has refused the frame otherwise)
      bool claimed;
      h = vox_find_or_claim(slots, mask, key, &claimed);
      atomicMax(&slots[h].seq, seq0 + vox_u64(k) + 1ULL);
      if (claimed) atomicAdd(&counters[0], 1ULL);
    }
    slot_of[k] = h;
  }
}

template <typename Frame>
__global__ __launch_bounds__(kVoxThreads) void k_vox_payload(Frame frame, long long i0, long long n, vox_u64 seq0, VoxSlot* slots, const unsigned* slot_of) {
  const long long stride = (long long)gridDim.x * kVoxThreads;
  for (long long k = (long long)blockIdx.x * kVoxThreads + threadIdx.x; k < n; k += stride) {
    const unsigned h = slot_of[k];
    if (h == kVoxNoSlot) continue;
    if (slots[h].seq != seq0 + vox_u64(k) + 1ULL) continue;
    double x, y, z, w;
    frame.load(i0 + k, x, y, z, w);
    slots[h].rec = make_float4(float(x), float(y), float(z), float(w));
  }
}

// ---- raw sensor_msgs/PointCloud2 records -> VoxFrameF64 (extract_raw_points, ros_cloud_converter.hpp:107-171) -----------------
// A record is `step` bytes; x y z (all float32 or all float64) and the intensity channel (uint8 / uint16 / uint32 / float32 /
// float64) sit at arbitrary byte offsets inside it -- 18- and 22-byte records exist, nothing is naturally aligned, so every
// field is put together from single bytes (little-endian) and never read through a typed pointer.  All conversions to double
// are exact.  Records of up to kVoxStageStep bytes: one workgroup per tile of kVoxThreads consecutive records, whose byte
// span is copied into LDS with 16-byte vector loads first -- the span is widened down / up to 16-byte boundaries; the raw
// buffer is 16-byte aligned and allocated to a multiple of 16 bytes, so the widened span stays inside it -- and the lanes
// pick their bytes from LDS.  Longer records (a lane would use a small part of what the tile stages) read their bytes from
// global memory directly.
enum { kPcUint8 = 2, kPcUint16 = 4, kPcUint32 = 6, kPcFloat32 = 7, kPcFloat64 = 8 };  // sensor_msgs/PointField datatypes
constexpr int kVoxStageStep = 128;
constexpr int kVoxStageVecs = kVoxThreads * kVoxStageStep / 16 + 2;  // a tile's span + up to 15 bytes before and after it

struct VoxCloud2 {
  const unsigned char* raw;  // num_points records of `step` bytes
  long long n;
  int step, ox, oy, oz, oi;  // byte offsets of x, y, z, intensity inside a record
};

template <int Bytes>
__device__ inline vox_u64 vox_le(const unsigned char* p) {
  vox_u64 v = 0;
#pragma unroll
  for (int k = 0; k < Bytes; k++) v |= vox_u64(p[k]) << (8 * k);
  return v;
}

template <int Type>
__device__ inline double vox_field(const unsigned char* p) {
  if constexpr (Type == kPcUint8) return double(p[0]);
  if constexpr (Type == kPcUint16) return double(unsigned(vox_le<2>(p)));
  if constexpr (Type == kPcUint32) return double(unsigned(vox_le<4>(p)));
  if constexpr (Type == kPcFloat32) return double(__uint_as_float(unsigned(vox_le<4>(p))));
  if constexpr (Type == kPcFloat64) return __longlong_as_double((long long)vox_le<8>(p));
}

template <int XyzType, int IntType, bool Staged>
__global__ __launch_bounds__(kVoxThreads) void k_vox_decode_cloud2(VoxCloud2 c, double4* pts, double* inten) {
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
      pts[i] = make_double4(vox_field<XyzType>(rec + c.ox), vox_field<XyzType>(rec + c.oy), vox_field<XyzType>(rec + c.oz), 0.0);
      inten[i] = vox_field<IntType>(rec + c.oi);
    }
  }
}

static __global__ __launch_bounds__(kVoxThreads) void k_vox_rehash(const VoxSlot* old_slots, long long old_cap, VoxSlot* slots, unsigned mask) {
  const long long stride = (long long)gridDim.x * kVoxThreads;
  for (long long s = (long long)blockIdx.x * kVoxThreads + threadIdx.x; s < old_cap; s += stride) {
    const VoxSlot v = old_slots[s];
    if (v.key == 0) continue;
    bool claimed;
    const unsigned h = vox_find_or_claim(slots, mask, v.key, &claimed);  // (keys are distinct: always a claim)
    slots[h].seq = v.seq;
    slots[h].rec = v.rec;
  }
}

// (seq + 1, slot) of every occupied slot, in arrival order -- the sort that follows fixes the order; *count += their number
static __global__ __launch_bounds__(kVoxThreads) void k_vox_compact(const VoxSlot* slots, long long cap, vox_u64* count, vox_u64* seq_out, unsigned* slot_out) {
  const long long stride = (long long)gridDim.x * kVoxThreads;
  for (long long s = (long long)blockIdx.x * kVoxThreads + threadIdx.x; s < cap; s += stride) {
    if (slots[s].key == 0) continue;
    const vox_u64 j = atomicAdd(count, 1ULL);
    seq_out[j] = slots[s].seq;
    slot_out[j] = unsigned(s);
  }
}

static __global__ __launch_bounds__(kVoxThreads) void k_vox_gather(const VoxSlot* slots, const vox_u64* seq_sorted, const unsigned* slot_sorted, long long m, float4* rec_out, long long* seq_out) {
  const long long stride = (long long)gridDim.x * kVoxThreads;
  for (long long j = (long long)blockIdx.x * kVoxThreads + threadIdx.x; j < m; j += stride) {
    rec_out[j] = slots[slot_sorted[j]].rec;
    seq_out[j] = (long long)(seq_sorted[j] - 1ULL);
  }
}

}  // namespace nidreg
