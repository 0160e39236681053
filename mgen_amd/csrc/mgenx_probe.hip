// mgenx_probe.hip -- memory-pattern probes of the diagnostics build (mgenx_diag_stream_read*,
// mgenx_diag_group_rw) and the probes of the per-flow passes' scan (mgenx_diag_blockscan,
// mgenx_diag_chunk_carry): no unpack code, and nothing at all in the product library.
#include "mgenx_internal.hpp"

#if MGENX_DIAG
#include "mgenx_blockscan.hpp"
#include "mgenx_diag.h"

namespace mgenx {

// Diagnostic: streaming read of `bytes` (16 B per lane per load, grid-stride), XOR-folded
// into one word per block so the loads are not dead.  Reference for achievable HBM rate.
__global__ void __launch_bounds__(256) stream_read_kernel(const u32x4_t* p, uint64_t n16,
                                                          uint32_t* out) {
  uint32_t acc = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n16; i += 4 * stride) {
    const u32x4_t a = p[i], b = p[i + stride], c = p[i + 2 * stride], d = p[i + 3 * stride];
    acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ d.x ^ d.y ^
           d.z ^ d.w;
  }
  for (; i < n16; i += stride) {
    const u32x4_t a = p[i];
    acc ^= a.x ^ a.y ^ a.z ^ a.w;
  }
  if (acc == 0x9E3779B9u) out[blockIdx.x] = acc;  // practically never taken
}

// Diagnostic: unpack_fixed_kernel's memory pattern alone (groups of 16 x 1 KiB dealt to waves
// round-robin, rows reloaded one group ahead, 512 B stored per group when MODE & 1).
template <int MODE>
__global__ void __launch_bounds__(1024) group_rw_kernel(const uint8_t* p, uint32_t n_groups,
                                                        uint8_t* out) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave_id = __builtin_amdgcn_readfirstlane(blockIdx.x * 16 + (threadIdx.x >> 6));
  const uint32_t n_waves = gridDim.x * 16;
  uint32_t g = wave_id;
  if (g >= n_groups) return;
  // lane l of row j: record l/4 of the group, bytes 64 j + 16 (l & 3)
  const uint32_t lo = (uint32_t)(lane >> 2) * 1024u + 16u * (lane & 3);
  u32x4_t d[16];
#pragma unroll
  for (int j = 0; j < 16; j++) d[j] = ldu128(p + (uint64_t)g * 16384u + lo + 64 * j);
  uint32_t acc = 0;
  while (g < n_groups) {
    const uint32_t gn = g + n_waves;
    const uint32_t gl = gn < n_groups ? gn : g;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      acc = (acc << 1) ^ d[j].x ^ d[j].y ^ d[j].z ^ d[j].w;
      __builtin_amdgcn_sched_barrier(0);
      d[j] = ldu128(p + (uint64_t)gl * 16384u + lo + 64 * j);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (MODE & 4) {  // 16-B stores from half the lanes
      if (lane < 32) {
        u32x4_t v = {acc, g, acc, g};
        *reinterpret_cast<u32x4_t*>(out + (uint64_t)g * 512u + 16u * lane) = v;
      }
    } else if (MODE & 1) {
      const uint64_t a = (uint64_t)out + (uint64_t)g * 512u + 8u * lane;
      const uint64_t v = (uint64_t)acc << 32 | g;
      if (MODE & 2) st_g64_wt(a, v); else st_g64(a, v);
    }
    g = gn;
  }
  if (!(MODE & 1) && acc == 0x9E3779B9u) out[lane] = 1;
}

// Diagnostic: group_rw with the row stores held back in registers and issued K groups at a
// time (K = 1 << LK), at each group's own row position; POL 0 = non-temporal, 1 = temporal,
// 2 = write-through stores.
template <int LK, int POL>
__global__ void __launch_bounds__(1024) group_rw_buf_kernel(const uint8_t* p, uint32_t n_groups,
                                                            uint8_t* out) {
  constexpr int K = 1 << LK;
  const int lane = threadIdx.x & 63;
  const uint32_t wave_id = __builtin_amdgcn_readfirstlane(blockIdx.x * 16 + (threadIdx.x >> 6));
  const uint32_t n_waves = gridDim.x * 16;
  uint32_t g = wave_id;
  if (g >= n_groups) return;
  const uint32_t lo = (uint32_t)(lane >> 2) * 1024u + 16u * (lane & 3);
  u32x4_t d[16];
#pragma unroll
  for (int j = 0; j < 16; j++) d[j] = ldu128(p + (uint64_t)g * 16384u + lo + 64 * j);
  uint32_t acc = 0;
  while (g < n_groups) {
    uint64_t buf[K];
    uint32_t gs[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
      const uint32_t gn = g + n_waves;
      const uint32_t gl = gn < n_groups ? gn : g;
#pragma unroll
      for (int j = 0; j < 16; j++) {
        acc = (acc << 1) ^ d[j].x ^ d[j].y ^ d[j].z ^ d[j].w;
        __builtin_amdgcn_sched_barrier(0);
        d[j] = ldu128(p + (uint64_t)gl * 16384u + lo + 64 * j);
        __builtin_amdgcn_sched_barrier(0);
      }
      buf[k] = (uint64_t)acc << 32 | g;
      gs[k] = g;
      g = gn;
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
      const uint64_t a = (uint64_t)out + (uint64_t)(gs[k] < n_groups ? gs[k] : 0u) * 512u + 8u * lane;
      if (POL == 0) st_g64_nt(a, buf[k]);
      else if (POL == 1) st_g64(a, buf[k]);
      else st_g64_wt(a, buf[k]);
    }
  }
}

// Diagnostic: every wave keeps the row stores of its (<= 16) groups in registers; RING rows
// in flight per wave (16 = one group ahead, 8 = half a group); BAR: a grid-wide arrival
// barrier (bounded spin) between the last read and the stores, so the chip reads, then
// writes.  POL as group_rw_buf_kernel.
template <int RING, bool BAR, int POL>
__global__ void __launch_bounds__(1024) group_rw_phase_kernel(const uint8_t* p, uint32_t n_groups,
                                                              uint8_t* out, uint32_t* counter) {
  constexpr int K = 16;
  const int lane = threadIdx.x & 63;
  const uint32_t wave_id = __builtin_amdgcn_readfirstlane(blockIdx.x * 16 + (threadIdx.x >> 6));
  const uint32_t n_waves = gridDim.x * 16;
  const uint32_t lo = (uint32_t)(lane >> 2) * 1024u + 16u * (lane & 3);
  const uint32_t my_groups = wave_id < n_groups ? (n_groups - wave_id + n_waves - 1) / n_waves : 0;
  // 32-bit byte offsets (slab < 4 GiB); group k of this wave, clamped to its last group
  auto goff = [&](int k) {
    const uint32_t kk = (uint32_t)k < my_groups ? (uint32_t)k : (my_groups ? my_groups - 1 : 0);
    const uint32_t g = wave_id + kk * n_waves;
    return (g < n_groups ? g : 0u) * 16384u + lo;
  };
  u32x4_t d[RING];
  uint32_t cur = goff(0), nxt = goff(1);
#pragma unroll
  for (int j = 0; j < RING; j++) d[j] = ldu128(p + (uint64_t)(cur + 64u * j));
  // a shift register of the last K groups' row words: buf[K-1] = the newest group
  uint64_t buf[K];
#pragma unroll
  for (int k = 0; k < K; k++) buf[k] = 0;
  uint32_t acc = 0;
  // two groups per trip keep the ring index static when RING does not divide 16
  for (uint32_t k = 0; k < my_groups; k++) {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      u32x4_t& x = d[j % RING];
      acc = (acc << 1) ^ x.x ^ x.y ^ x.z ^ x.w;
      __builtin_amdgcn_sched_barrier(0);
      const int jn = j + RING;  // row r + RING: this group or the next
      x = ldu128(p + (uint64_t)(jn < 16 ? cur + 64u * jn : nxt + 64u * (jn - 16)));
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int q = 0; q < K - 1; q++) buf[q] = buf[q + 1];
    buf[K - 1] = (uint64_t)acc << 32 | k;
    cur = nxt;
    nxt = goff((int)k + 2);
  }
#pragma unroll
  for (int k = 0; k < K; k++) {  // buf[k] holds group my_groups - K + k
    const int kg = (int)my_groups - K + k;
    const uint32_t g = wave_id + (uint32_t)kg * n_waves;
    if (kg >= 0 && g < n_groups) {
      const uint64_t a = (uint64_t)out + (uint64_t)g * 512u + 8u * lane;
      if (POL == 0) st_g64_nt(a, buf[k]);
      else if (POL == 1) st_g64(a, buf[k]);
      else st_g64_wt(a, buf[k]);
    }
  }
}

hipError_t launch_group_rw(const uint8_t* p, uint64_t bytes, uint8_t* out, int mode, int grid,
                           hipStream_t stream) {
  const uint32_t ng = (uint32_t)(bytes / 16384);
  if (mode >= 4096) {  // 4096 + 16 * ring_sel + 4 * bar + pol
    static DevBuf counter_buf;  // (kept for the life of the process)
    uint32_t* counter = static_cast<uint32_t*>(counter_buf.get(256));
    if (!counter) return hipErrorOutOfMemory;
    hipError_t e = hipMemsetAsync(counter, 0, 16, stream);
    if (e != hipSuccess) return e;
    const int m = mode - 4096;
#define MGENX_GPH(RING, BAR, POL, CODE)                                                         \
  if (m == CODE) {                                                                              \
    hipLaunchKernelGGL((group_rw_phase_kernel<RING, BAR, POL>), dim3(grid), dim3(1024), 0, stream, \
                       p, ng, out, counter);                                                    \
    return hipGetLastError();                                                                   \
  }
    MGENX_GPH(16, false, 0, 0) MGENX_GPH(16, true, 0, 4) MGENX_GPH(8, false, 0, 16)
    MGENX_GPH(8, true, 0, 20) MGENX_GPH(16, true, 1, 5) MGENX_GPH(8, true, 1, 21)
#undef MGENX_GPH
    return hipErrorInvalidValue;
  }
  if (mode >= 16) {
    const int lk = ((mode >> 4) & 7) - 1, pol = (mode >> 8) & 3;
#define MGENX_GRB(LK, POL)                                                                   \
  if (lk == LK && pol == POL) {                                                              \
    hipLaunchKernelGGL((group_rw_buf_kernel<LK, POL>), dim3(grid), dim3(1024), 0, stream, p, ng, \
                       out);                                                                 \
    return hipGetLastError();                                                                \
  }
    MGENX_GRB(0, 0) MGENX_GRB(1, 0) MGENX_GRB(2, 0) MGENX_GRB(3, 0) MGENX_GRB(4, 0)
    MGENX_GRB(2, 1) MGENX_GRB(4, 1) MGENX_GRB(2, 2) MGENX_GRB(4, 2)
#undef MGENX_GRB
    return hipErrorInvalidValue;
  }
  switch (mode & 7) {
    case 4: hipLaunchKernelGGL(group_rw_kernel<4>, dim3(grid), dim3(1024), 0, stream, p, ng, out); break;
    case 0: hipLaunchKernelGGL(group_rw_kernel<0>, dim3(grid), dim3(1024), 0, stream, p, ng, out); break;
    case 1: hipLaunchKernelGGL(group_rw_kernel<1>, dim3(grid), dim3(1024), 0, stream, p, ng, out); break;
    default: hipLaunchKernelGGL(group_rw_kernel<3>, dim3(grid), dim3(1024), 0, stream, p, ng, out); break;
  }
  return hipGetLastError();
}

// Diagnostic: a coalesced read of `bytes` at W bytes per lane (4, 8 or 24: the access shapes of
// the config-4 kernels' column loads and 24-B record loads) -- FETCH_SIZE calibration per shape.
struct alignas(8) SrW24 {
  uint32_t w[6];
};
__device__ __forceinline__ uint32_t sr_fold(uint32_t v) { return v; }
__device__ __forceinline__ uint32_t sr_fold(uint2 v) { return v.x ^ v.y; }
__device__ __forceinline__ uint32_t sr_fold(const SrW24& v) {
  return v.w[0] ^ v.w[1] ^ v.w[2] ^ v.w[3] ^ v.w[4] ^ v.w[5];
}
template <typename T>
__global__ void __launch_bounds__(256) stream_read_w_kernel(const T* p, uint64_t n, uint32_t* out) {
  uint32_t acc = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    const T a = p[i], b = p[i + stride], c = p[i + 2 * stride], d = p[i + 3 * stride];
    acc ^= sr_fold(a) ^ sr_fold(b) ^ sr_fold(c) ^ sr_fold(d);
  }
  for (; i < n; i += stride) acc ^= sr_fold(p[i]);
  if (acc == 0x9E3779B9u) out[blockIdx.x] = acc;  // practically never taken
}
hipError_t launch_stream_read_w(const uint8_t* p, uint64_t bytes, uint32_t* out, int grid,
                                int width, hipStream_t stream) {
  if (width == 4)
    hipLaunchKernelGGL(stream_read_w_kernel<uint32_t>, dim3(grid), dim3(256), 0, stream,
                       reinterpret_cast<const uint32_t*>(p), bytes / 4, out);
  else if (width == 8)
    hipLaunchKernelGGL(stream_read_w_kernel<uint2>, dim3(grid), dim3(256), 0, stream,
                       reinterpret_cast<const uint2*>(p), bytes / 8, out);
  else if (width == 24)
    hipLaunchKernelGGL(stream_read_w_kernel<SrW24>, dim3(grid), dim3(256), 0, stream,
                       reinterpret_cast<const SrW24*>(p), bytes / 24, out);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_stream_read(const uint8_t* p, uint64_t bytes, uint32_t* out, int grid,
                              hipStream_t stream) {
  hipLaunchKernelGGL(stream_read_kernel, dim3(grid), dim3(256), 0, stream,
                     reinterpret_cast<const u32x4_t*>(p), bytes / 16, out);
  return hipGetLastError();
}

// Diagnostic: mgenx_blockscan.hpp's scan and carry loop alone, one workgroup
// (mgenx_diag_blockscan, mgenx_diag_chunk_carry; include/mgenx_diag.h).
struct ScanProbe {  // the widest value in use (mgenx_match.hip's MatchAcc): 96 B
  uint64_t f[12];   // field k: k % 3 == 0 a wrapping sum, 1 a signed minimum, 2 a signed maximum
  static __device__ __forceinline__ ScanProbe of(ScanProbe a, const ScanProbe& b) {
#pragma unroll
    for (int k = 0; k < 12; k++) {
      const int64_t x = (int64_t)a.f[k], y = (int64_t)b.f[k];
      const uint64_t m = k % 3 == 1 ? (x < y ? x : y) : (x > y ? x : y);
      a.f[k] = k % 3 == 0 ? a.f[k] + b.f[k] : m;
    }
    return a;
  }
};
__device__ __forceinline__ uint32_t scan_probe_value(uint32_t in, uint32_t*) { return in; }
__device__ __forceinline__ int64_t scan_probe_value(int64_t in, int64_t*) { return in; }
__device__ __forceinline__ ScanProbe scan_probe_value(uint64_t in, ScanProbe*) {
  ScanProbe v;
#pragma unroll
  for (int k = 0; k < 12; k++) v.f[k] = in * (uint64_t)(2 * k + 1) + (uint64_t)k;
  return v;
}

// one kernel per kind and per use of `open`, as the callers compile the scan: the 96-B value
// keeps its registers to itself
template <class Op, bool kSync, bool kOpen, class In, class V>
__global__ void __launch_bounds__(kChunk)
blockscan_probe_kernel(const In* val, const uint32_t* head, V* out, uint32_t* open_out) {
  __shared__ V s_v[kWaves];
  __shared__ uint32_t s_h[kWaves];
  const uint32_t t = threadIdx.x;
  const V v = scan_probe_value(val[t], (V*)nullptr);
  bool open = false;
  out[t] = seg_scan<Op, kSync>(v, head[t] != 0u, s_v, s_h, kOpen ? &open : nullptr);
  if (kOpen) open_out[t] = open ? 1u : 0u;
}
template <class Op, bool kSync, class In, class V>
hipError_t launch_blockscan_probe(const void* val, const uint32_t* head, void* out,
                                  uint32_t* open_out, hipStream_t stream) {
  if (open_out)
    hipLaunchKernelGGL((blockscan_probe_kernel<Op, kSync, true, In, V>), dim3(1), dim3(kChunk), 0,
                       stream, (const In*)val, head, (V*)out, open_out);
  else
    hipLaunchKernelGGL((blockscan_probe_kernel<Op, kSync, false, In, V>), dim3(1), dim3(kChunk), 0,
                       stream, (const In*)val, head, (V*)out, open_out);
  return hipGetLastError();
}

template <class Op, class V>
__device__ __forceinline__ void carry_probe(const V* val, const uint32_t* head, uint32_t n, V idle,
                                            V* out) {
  __shared__ V s_v[kWaves];
  __shared__ uint32_t s_h[kWaves];
  __shared__ V s_run;
  chunk_carry<Op>(
      n, idle,
      [&](uint32_t c, V& v) {
        v = val[c];
        return head && head[c] != 0u;
      },
      [&](uint32_t c, V v) { out[c] = v; }, s_v, s_h, &s_run);
}

__global__ void __launch_bounds__(kChunk)
chunk_carry_probe_kernel(int kind, const void* val, const uint32_t* head, uint32_t n, void* out) {
  if (kind == 0)
    carry_probe<SumOp>((const uint32_t*)val, head, n, 0u, (uint32_t*)out);
  else if (kind == 1)
    carry_probe<MaxOp>((const int64_t*)val, head, n, (int64_t)INT64_MIN, (int64_t*)out);
  else
    carry_probe<SumOp>((const uint32_t*)val, (const uint32_t*)nullptr, n, 0u, (uint32_t*)out);
}

}  // namespace mgenx

extern "C" int mgenx_diag_blockscan(int kind, const void* dev_val, const uint32_t* dev_head,
                                    void* dev_out, uint32_t* dev_open, void* stream) {
  if (kind < 0 || kind > 2 || !dev_val || !dev_head || !dev_out) return MGENX_EINVAL;
  using namespace mgenx;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e =
      kind == 0 ? launch_blockscan_probe<SumOp, true, uint32_t, uint32_t>(dev_val, dev_head,
                                                                          dev_out, dev_open, s)
      : kind == 1 ? launch_blockscan_probe<MaxOp, true, int64_t, int64_t>(dev_val, dev_head,
                                                                          dev_out, dev_open, s)
                  : launch_blockscan_probe<ScanProbe, false, uint64_t, ScanProbe>(
                        dev_val, dev_head, dev_out, dev_open, s);
  return e == hipSuccess ? MGENX_OK : MGENX_EDEVICE;
}

extern "C" int mgenx_diag_chunk_carry(int kind, const void* dev_val, const uint32_t* dev_head,
                                      uint32_t n, void* dev_out, void* stream) {
  if (kind < 0 || kind > 2 || (n && (!dev_val || !dev_out || (kind != 2 && !dev_head))))
    return MGENX_EINVAL;
  hipLaunchKernelGGL(mgenx::chunk_carry_probe_kernel, dim3(1), dim3(mgenx::kChunk), 0,
                     (hipStream_t)stream, kind, dev_val, dev_head, n, dev_out);
  return hipGetLastError() == hipSuccess ? MGENX_OK : MGENX_EDEVICE;
}
#endif  // MGENX_DIAG
