// Device-side building blocks of the batched kernels: the bbhash64 tile
// helpers, the prefix search, and the tile walk shared by the hash-only
// kernel, the fused copy+digest kernel (digest.hip) and the striped
// copy+digest kernel (stripe.hip); batched_copy in memops.hip uses the
// search. Spec: csrc/include/blackbird/gpu/digest_spec.h.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "blackbird/gpu/digest_spec.h"
#include "blackbird/gpu/gpu_kernels.h"

namespace blackbird::gpu::dev {

using i32x4 = __attribute__((__vector_size__(16))) int;
using i32x16 = __attribute__((__vector_size__(64))) int;
using namespace blackbird::digest;

constexpr int kBlock = 256;  // 4 waves
constexpr int kWavesPerBlock = kBlock / 64;

// Largest i with prefix[i] <= c (prefix is non-decreasing, prefix[0] == 0).
__device__ inline uint32_t find_seg(const uint64_t* __restrict__ prefix,
                                    uint32_t n, uint64_t c) {
  uint32_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Per-lane B fragment: 16 bytes B[k][c] with c = lane&31, k = (lane>>5)*16+j.
__device__ inline i32x4 make_b_frag(int lane) {
  union {
    int8_t b[16];
    i32x4 v;
  } u;
  const int c = lane & 31;
  const int k0 = (lane >> 5) * 16;
#pragma unroll
  for (int j = 0; j < 16; ++j) u.b[j] = b_matrix(k0 + j, c);
  return u.v;
}

// Each lane folds a FIXED set of 16 (row,col) positions; weights precomputed
// into registers once.
struct WReg {
  uint32_t w[16];
};

__device__ inline WReg make_w_reg(int lane) {
  WReg r;
  const int col = lane & 31;
  const int rbase = 4 * (lane >> 5);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int row = (j & 3) + 8 * (j >> 2) + rbase;
    r.w[j] = w_weight(row * 32 + col);
  }
  return r;
}

// The spec's group fold f(t,g) of this lane's 16 accumulators. It does not
// depend on where the tile sits; position enters only through mix_slot.
__device__ inline uint64_t fold_group(const i32x16& acc, const WReg& wr) {
  uint64_t f = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t c32 = static_cast<uint32_t>(acc[j]);
    f += static_cast<uint64_t>(c32) * static_cast<uint64_t>(wr.w[j]);
  }
  return f;
}

__device__ inline uint64_t mix_slot(uint64_t f, uint64_t slot) {
  return mix64(f + tile_weight(slot));
}

__device__ inline uint64_t fold_tile(const i32x16& acc, const WReg& wr,
                                     uint64_t slot) {
  return mix_slot(fold_group(acc, wr), slot);
}

// Lane's 16-byte offset within a 1024-B tile for the MFMA A-fragment map
// ((lane&31)*32 + (lane>>5)*16) — the wave covers the tile exactly once and
// the accesses stay fully coalesced.
__device__ inline uint32_t lane_tile_offset(int lane) {
  return (lane & 31) * 32 + (lane >> 5) * 16;
}

__device__ inline i32x4 load_a_frag(const uint8_t* tile_base, int lane) {
  return *reinterpret_cast<const i32x4*>(tile_base + lane_tile_offset(lane));
}

__device__ inline i32x4 load_a_frag_guarded(const uint8_t* base, uint64_t tile_off,
                                            uint64_t nbytes, int lane) {
  union {
    int8_t b[16];
    i32x4 v;
  } u;
  const uint64_t lane_off = tile_off + lane_tile_offset(lane);
#pragma unroll
  for (int j = 0; j < 16; ++j)
    u.b[j] = (lane_off + j < nbytes) ? static_cast<int8_t>(base[lane_off + j]) : 0;
  return u.v;
}

__device__ inline uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_down(static_cast<unsigned long long>(v), off, 64);
  return v;
}

// One MFMA and one group fold: everything of a tile's hash but its position.
__device__ inline uint64_t fold_tile_frag(const i32x4& a_frag,
                                          const i32x4& b_frag, const WReg& wr) {
  i32x16 acc = {};
  acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a_frag, b_frag, acc, 0, 0, 0);
  return fold_group(acc, wr);
}

__device__ inline uint64_t hash_tile_frag(const i32x4& a_frag,
                                          const i32x4& b_frag, const WReg& wr,
                                          uint64_t slot) {
  return mix_slot(fold_tile_frag(a_frag, b_frag, wr), slot);
}

// The batched tile walk. One desc = one contiguous run of bytes that starts
// on a tile boundary: a whole object at object-offset 0 (CopyDesc), or a
// segment of a striped object (StripeSeg). tile_prefix[i] is the global index
// of desc i's first 1-KiB tile. Each wave owns a CONTIGUOUS range of global
// tiles, so desc switches (a 64-lane reduction + one atomic) happen only at
// desc boundaries inside the range; the current descriptor/boundary live in
// registers (a per-tile global load of descs[]/tile_prefix[] serializes on
// L2 latency). Every tile is loaded once with the MFMA A-fragment lane map
// (fully coalesced) and hashed in registers; out[i] accumulates desc i's
// partial sums and is finalized by a follow-up kernel.
//   kCopy:     also store the fragment to dst with the same lane map.
//   kPrefetch: software pipeline — the NEXT full tile's fragment loads while
//              the current one is stored+hashed, so the VALU fold hides the
//              load latency.
//   StripeSeg: the tile's group fold feeds two sums — out[i], slots counted
//              from the segment's start, and obj_out[seg.obj], slots counted
//              from the object's start (all 64-bit). A segment at tile 0 of
//              its object has the same slots in both, so it runs one mix per
//              tile and adds its one sum to both accumulators.
template <bool kCopy, bool kPrefetch, typename Desc>
__device__ __forceinline__ void digest_walk(
    const Desc* __restrict__ descs, const uint64_t* __restrict__ tile_prefix,
    uint32_t nobjs, uint64_t total_tiles, unsigned long long* __restrict__ out,
    unsigned long long* __restrict__ obj_out = nullptr) {
  constexpr bool kStripe = std::is_same_v<Desc, StripeSeg>;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const uint64_t gwave =
      static_cast<uint64_t>(blockIdx.x) * kWavesPerBlock + wave;
  const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * kWavesPerBlock;
  const uint64_t per = (total_tiles + nwaves - 1) / nwaves;
  const uint64_t begin = gwave * per;
  const uint64_t end = begin + per < total_tiles ? begin + per : total_tiles;
  if (begin >= total_tiles) return;

  const i32x4 b_frag = make_b_frag(lane);
  const WReg wr = make_w_reg(lane);
  const uint32_t lane_off = lane_tile_offset(lane);

  uint32_t oi = find_seg(tile_prefix, nobjs, begin);
  const uint8_t* src;
  uint8_t* dst;
  uint64_t nbytes, cur_full;
  [[maybe_unused]] uint64_t first_slot = 0;  // StripeSeg: first_tile * 64
  [[maybe_unused]] uint32_t obj = 0;
  auto enter_object = [&] {
    const Desc d = descs[oi];
    src = static_cast<const uint8_t*>(d.src);
    dst = static_cast<uint8_t*>(d.dst);
    nbytes = d.nbytes;
    cur_full = nbytes / kTileBytes;
    if constexpr (kStripe) {
      first_slot = d.first_tile * 64;
      obj = d.obj;
    }
  };
  enter_object();
  uint64_t base_tile = tile_prefix[oi];
  uint64_t next_boundary = (oi + 1 < nobjs) ? tile_prefix[oi + 1] : ~0ull;

  uint64_t h = 0;
  [[maybe_unused]] uint64_t ho = 0;  // StripeSeg: the object-slot sum
  // StripeSeg, leaving a segment after h was reduced: the object's share
  [[maybe_unused]] auto flush_object = [&] {
    if (first_slot != 0) ho = wave_sum_u64(ho);  // wave-uniform
    else ho = h;
    if (lane == 0 && ho != 0) atomicAdd(&obj_out[obj], ho);
    ho = 0;
  };
  bool have_pre = false;
  i32x4 pre{};
  for (uint64_t gt = begin; gt < end; ++gt) {
    while (gt >= next_boundary) {
      h = wave_sum_u64(h);
      if (lane == 0 && h != 0) atomicAdd(&out[oi], h);
      if constexpr (kStripe) flush_object();
      h = 0;
      ++oi;
      enter_object();
      base_tile = next_boundary;
      next_boundary = (oi + 1 < nobjs) ? tile_prefix[oi + 1] : ~0ull;
      have_pre = false;  // prefetch belonged to the previous object
    }
    const uint64_t t = gt - base_tile;
    const uint64_t toff = t * kTileBytes;
    i32x4 a;
    if (t < cur_full) {
      if constexpr (kPrefetch) {
        a = have_pre ? pre : load_a_frag(src + toff, lane);
        have_pre = (gt + 1 < end) && (gt + 1 < next_boundary) &&
                   (t + 1 < cur_full);
        if (have_pre) pre = load_a_frag(src + toff + kTileBytes, lane);
      } else {
        a = load_a_frag(src + toff, lane);
      }
      // nontemporal: an A/B test against a temporal (L2-filling) store was
      // within run variance end-to-end; the 1000-step soak record stands on
      // this version
      if constexpr (kCopy)
        __builtin_nontemporal_store(
            a, reinterpret_cast<i32x4*>(dst + toff + lane_off));
    } else {
      // tail tile: zero-padded hash, byte-guarded store
      a = load_a_frag_guarded(src, toff, nbytes, lane);
      if constexpr (kCopy) {
        const uint64_t base = toff + lane_off;
        const int8_t* ab = reinterpret_cast<const int8_t*>(&a);
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (base + j < nbytes) dst[base + j] = static_cast<uint8_t>(ab[j]);
      }
    }
    const uint64_t slot = t * 64 + lane;
    if constexpr (kStripe) {
      const uint64_t f = fold_tile_frag(a, b_frag, wr);
      h += mix_slot(f, slot);
      if (first_slot != 0) ho += mix_slot(f, first_slot + slot);  // wave-uniform
    } else {
      h += hash_tile_frag(a, b_frag, wr, slot);
    }
  }
  h = wave_sum_u64(h);
  if (lane == 0 && h != 0) atomicAdd(&out[oi], h);
  if constexpr (kStripe) flush_object();
}

}  // namespace blackbird::gpu::dev
