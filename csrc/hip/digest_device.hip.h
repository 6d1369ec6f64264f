// Device-side building blocks of the batched kernels: the bbhash64 tile
// helpers, the prefix search, and the tile walks. One range rule
// (wave_tile_range), one boundary loop (walk_descs) and one pipelined run
// (run_tiles) serve both: digest_walk (the hash-only and fused copy+digest
// kernels of digest.hip, the striped one of stripe.hip) and patch_walk
// (patch.hip) add what they do with a tile and with a descriptor's sums.
// batched_copy in memops.hip uses the search.
// Spec: csrc/include/blackbird/gpu/digest_spec.h.
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

// Each lane folds a FIXED set of 16 (row,col) positions with weights it keeps
// in registers.
struct WReg {
  uint32_t w[16];
};

// What a lane needs of the spec's two constant matrices, lane-major, built at
// compile time: a wave fetches its constants with five 16-byte loads per lane
// where hashing them costs it 32 splitmix64 per lane (some 480 vector
// instructions) before its first payload load.
//   b[lane]: the MFMA B fragment, B[k][c] with c = lane&31, k = (lane>>5)*16+j
//   w[lane]: the fold weights W[row*32+col] of the lane's 16 accumulators in
//            the MFMA C layout: col = lane&31, row = (j&3)+8*(j>>2)+4*(lane>>5)
struct LaneTables {
  alignas(16) int8_t b[64][16];
  alignas(16) uint32_t w[64][16];
};

constexpr LaneTables make_lane_tables() {
  LaneTables t{};
  for (int lane = 0; lane < 64; ++lane) {
    const int col = lane & 31;
    const int k0 = (lane >> 5) * 16;
    const int rbase = 4 * (lane >> 5);
    for (int j = 0; j < 16; ++j) {
      const int row = (j & 3) + 8 * (j >> 2) + rbase;
      t.b[lane][j] = b_matrix(k0 + j, col);
      t.w[lane][j] = w_weight(row * 32 + col);
    }
  }
  return t;
}

// The C-layout map above against the spec's own fold groups: lane g folds
// group g, element j.
constexpr bool lane_tables_match_spec(const LaneTables& t) {
  for (int g = 0; g < 64; ++g)
    for (int j = 0; j < 16; ++j) {
      if (t.w[g][j] != w_weight(fold_row(g, j) * 32 + fold_col(g))) return false;
      if (t.b[g][j] != b_matrix((g >> 5) * 16 + j, fold_col(g))) return false;
    }
  return true;
}

inline constexpr LaneTables kLaneTablesImage = make_lane_tables();
static_assert(lane_tables_match_spec(kLaneTablesImage));
static_assert(sizeof(LaneTables) == 64 * 16 + 64 * 64);

static __device__ const LaneTables kLaneTables = kLaneTablesImage;

__device__ inline i32x4 load_b_frag(int lane) {
  return *reinterpret_cast<const i32x4*>(kLaneTables.b[lane]);
}

__device__ inline WReg load_w_reg(int lane) {
  WReg r;
  const i32x4* row = reinterpret_cast<const i32x4*>(kLaneTables.w[lane]);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const i32x4 v = row[q];
#pragma unroll
    for (int k = 0; k < 4; ++k) r.w[4 * q + k] = static_cast<uint32_t>(v[k]);
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

// Payload bytes are always global memory: local HBM, IPC-mapped peer memory
// or GPU-mapped host memory. Descriptors carry them as generic pointers;
// going through address space 1 lets the compiler emit global_load/
// global_store (one counter, in-order return, counted waits) instead of flat
// accesses, which it may only ever wait out completely.
template <typename T>
using global_ptr = __attribute__((address_space(1))) T*;

__device__ inline global_ptr<const uint8_t> as_global(const uint8_t* p) {
  return (global_ptr<const uint8_t>)p;
}
__device__ inline global_ptr<uint8_t> as_global(uint8_t* p) {
  return (global_ptr<uint8_t>)p;
}

// Values every lane of the wave holds alike, moved to scalar registers so
// that what is computed and branched on from them stays scalar.
__device__ inline uint32_t wave_uniform(uint32_t v) {
  return __builtin_amdgcn_readfirstlane(v);
}
__device__ inline uint64_t wave_uniform(uint64_t v) {
  const uint32_t lo = wave_uniform(static_cast<uint32_t>(v));
  const uint32_t hi = wave_uniform(static_cast<uint32_t>(v >> 32));
  return (static_cast<uint64_t>(hi) << 32) | lo;
}
template <typename T>
__device__ inline T* wave_uniform(T* p) {
  return reinterpret_cast<T*>(wave_uniform(reinterpret_cast<uint64_t>(p)));
}

// tile_base is wave-uniform; lane_off = lane_tile_offset(lane). kNt: the
// load is nontemporal, as the copy's stores are: a copied tile is not read
// again.
template <bool kNt = false>
__device__ inline i32x4 load_a_frag(const uint8_t* tile_base, uint32_t lane_off) {
  const auto p = (global_ptr<const i32x4>)(as_global(tile_base) + lane_off);
  if constexpr (kNt) return __builtin_nontemporal_load(p);
  else return *p;
}

// kNt: the store is nontemporal, the default of every copying walk: what it
// writes is not expected to be read soon. A plain store allocates in the
// 256 MiB Infinity Cache, and measurably so (profiles/warm_tail_checks.md):
// on the 512 x 1 MiB put, the last 128 MiB stored plainly make that launch
// 9 us shorter and, loaded plainly, the get behind it 9 us shorter; with two
// lanes the pair gains 5 %. Stored plainly throughout, the put is 23 us
// shorter and the get no faster than cold: the batch evicts itself. Hence
// the walk's warm tail (digest_walk, kWarm), and nontemporal everywhere else.
template <bool kNt = true>
__device__ inline void store_a_frag(uint8_t* tile_base, uint32_t lane_off,
                                    const i32x4& a) {
  const auto p = (global_ptr<i32x4>)(as_global(tile_base) + lane_off);
  if constexpr (kNt) __builtin_nontemporal_store(a, p);
  else *p = a;
}

// The tail tile: bytes at and past nbytes read as zero ...
__device__ inline i32x4 load_a_frag_guarded(const uint8_t* base, uint64_t tile_off,
                                            uint64_t nbytes, uint32_t lane_off) {
  union {
    int8_t b[16];
    i32x4 v;
  } u;
  const global_ptr<const uint8_t> g = as_global(base);
  const uint64_t off = tile_off + lane_off;
#pragma unroll
  for (int j = 0; j < 16; ++j)
    u.b[j] = (off + j < nbytes) ? static_cast<int8_t>(g[off + j]) : 0;
  return u.v;
}

// ... and are not written.
__device__ inline void store_a_frag_guarded(uint8_t* base, uint64_t tile_off,
                                            uint64_t nbytes, uint32_t lane_off,
                                            const i32x4& a) {
  const global_ptr<uint8_t> g = as_global(base);
  const uint64_t off = tile_off + lane_off;
  const int8_t* ab = reinterpret_cast<const int8_t*>(&a);
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (off + j < nbytes) g[off + j] = static_cast<uint8_t>(ab[j]);
}

// The windowed pair of an edge tile (patch_edge_tile): tile positions
// [lo, hi) take the bytes at src, src[0] being position lo; every other
// position keeps the lane's byte of `old`. Nothing of src is read outside
// [src, src + hi - lo).
__device__ inline i32x4 compose_a_frag_windowed(const i32x4& old,
                                                const uint8_t* src, uint32_t lo,
                                                uint32_t hi, uint32_t lane_off) {
  union {
    int8_t b[16];
    i32x4 v;
  } u;
  u.v = old;
  const global_ptr<const uint8_t> g = as_global(src);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t p = lane_off + j;
    if (p >= lo && p < hi) u.b[j] = static_cast<int8_t>(g[p - lo]);
  }
  return u.v;
}

// ... and only the positions [lo, hi) are written.
__device__ inline void store_a_frag_windowed(uint8_t* tile, uint32_t lo,
                                             uint32_t hi, uint32_t lane_off,
                                             const i32x4& a) {
  const global_ptr<uint8_t> g = as_global(tile);
  const int8_t* ab = reinterpret_cast<const int8_t*>(&a);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t p = lane_off + j;
    if (p >= lo && p < hi) g[p] = static_cast<uint8_t>(ab[j]);
  }
}

__device__ inline uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_down(static_cast<unsigned long long>(v), off, 64);
  return v;
}

// The tile's projection A_t × B: one MFMA.
__device__ inline i32x16 project_tile(const i32x4& a_frag, const i32x4& b_frag) {
  const i32x16 zero = {};
  return __builtin_amdgcn_mfma_i32_32x32x32_i8(a_frag, b_frag, zero, 0, 0, 0);
}

// One MFMA and one group fold: everything of a tile's hash but its position.
__device__ inline uint64_t fold_tile_frag(const i32x4& a_frag,
                                          const i32x4& b_frag, const WReg& wr) {
  return fold_group(project_tile(a_frag, b_frag), wr);
}

__device__ inline uint64_t hash_tile_frag(const i32x4& a_frag,
                                          const i32x4& b_frag, const WReg& wr,
                                          uint64_t slot) {
  return mix_slot(fold_tile_frag(a_frag, b_frag, wr), slot);
}

// Full tiles whose loads a copying wave keeps in flight while it folds the
// current one. Measured at 1..4 on the 512 × 1 MiB put
// (profiles/walk_pipeline_checks.md).
constexpr int kWalkDepth = 4;

// Longest run of full tiles a walk takes in one go (1 TiB).
constexpr uint32_t kMaxRun = 1u << 30;

// The range rule of every batched walk: each wave owns one CONTIGUOUS range
// [begin, end) of the launch's global tiles, total_tiles split evenly over
// the waves of the grid (sized by the host: digest_grid). False: none is left
// for this wave. The wave index and all that follows from it are the same in
// every lane, and the compiler is told so.
__device__ inline bool wave_tile_range(uint64_t total_tiles, uint64_t& begin,
                                       uint64_t& end) {
  const uint32_t wave = wave_uniform(threadIdx.x >> 6);
  const uint64_t gwave =
      static_cast<uint64_t>(blockIdx.x) * kWavesPerBlock + wave;
  const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * kWavesPerBlock;
  const uint64_t per = (total_tiles + nwaves - 1) / nwaves;
  begin = gwave * per;
  end = begin + per < total_tiles ? begin + per : total_tiles;
  return begin < total_tiles;
}

// The boundary loop of every batched walk. One desc = one contiguous run of
// bytes that starts on a tile boundary; tile_prefix[i] is the global index of
// desc i's first 1-KiB tile. The global tiles [begin, end), begin < end, are
// cut into runs of full tiles of one desc plus at most one tail tile per
// desc, so desc switches happen only at desc boundaries inside the range.
// The current desc and its boundaries live in scalar registers (a per-tile
// global load of descs[]/tile_prefix[] serializes on L2 latency). The walk
// brings:
//   enter(d)         desc d is the current one from here on; returns its
//                    wave-uniform byte count
//   leave(i)         the range holds no more of desc i: flush its sums
//   full_run(t0, n)  n >= 1 full tiles of the current desc, from its tile t0
//   tail_tile(t)     the current desc's last tile t, not a full one
template <typename Desc, typename Enter, typename Leave, typename FullRun,
          typename TailTile>
__device__ __forceinline__ void walk_descs(
    const Desc* __restrict__ descs, const uint64_t* __restrict__ tile_prefix,
    uint32_t n, uint64_t begin, uint64_t end, Enter&& enter, Leave&& leave,
    FullRun&& full_run, TailTile&& tail_tile) {
  uint32_t i = wave_uniform(find_seg(tile_prefix, n, begin));
  uint64_t cur_full, base_tile, next_boundary;
  auto enter_desc = [&] {
    cur_full = enter(descs[i]) / kTileBytes;
    next_boundary = (i + 1 < n) ? wave_uniform(tile_prefix[i + 1]) : ~0ull;
  };
  enter_desc();
  base_tile = wave_uniform(tile_prefix[i]);

  uint64_t gt = begin;
  while (gt < end) {
    while (gt >= next_boundary) {
      leave(i);
      ++i;
      base_tile = next_boundary;
      enter_desc();
    }
    const uint64_t t = gt - base_tile;
    // the desc's tiles inside this wave's range, and the full ones of them
    const uint64_t stop =
        (end < next_boundary ? end : next_boundary) - base_tile;
    const uint64_t full_stop = stop < cur_full ? stop : cur_full;
    if (t < full_stop) {
      const uint64_t left = full_stop - t;
      const uint32_t run = left < kMaxRun ? static_cast<uint32_t>(left) : kMaxRun;
      full_run(t, run);
      gt += run;
    } else {
      tail_tile(t);
      ++gt;
    }
  }
  leave(i);
}

// The pipelined run of every batched walk: n >= 1 full tiles of the current
// desc, from its tile t0, kDepth tiles deep (0: load, then fold). Counting
// inside a run is 32-bit: scalar compares, where 64-bit ones take the VALU.
// The walk brings, each for the desc's tile t:
//   load(t)        -> Slot: issue the tile's loads
//   consume(s, t)  the fragments' last uses, the store and the MFMAs; returns
//                  the projections
//   fold(acc, t)   the long VALU part of the hash
// t0 is added HERE. Handed the count alone, with t0 added in the callables,
// the compiler splits a slot into a scalar part and (k*64 | lane) and keeps
// the latter in registers throughout: 6 VGPRs, an occupancy step of the put
// and get kernels (profiles/walk_skeleton_checks.md).
template <int kDepth, typename Slot, typename Load, typename Consume,
          typename Fold>
__device__ __forceinline__ void run_tiles(uint64_t t0, uint32_t n, Load&& load,
                                          Consume&& consume, Fold&& fold) {
  // tiles [i, stop) of the run one by one: load, consume, fold
  auto plain = [&](uint32_t i, uint32_t stop) {
    for (; i < stop; ++i) fold(consume(load(t0 + i), t0 + i), t0 + i);
  };
  // no pipeline, or a run too short for one
  if (kDepth == 0 || n < 2u * kDepth) {
    plain(0, n);
    return;
  }
  if constexpr (kDepth > 0) {
    // buf[k] holds tile i+k, then tile i+k+kDepth: the slots rotate by
    // unrolling, no fragment is ever moved between registers.
    Slot buf[kDepth];
    // One step: consume tile i+k, refill its slot kDepth tiles ahead, then
    // the long fold. The scheduling barriers keep that order. A load
    // hoisted above the consumption needs a second register set, and the
    // copy back into the slot waits for the load it was meant to leave in
    // flight; loads issued in another order than their slots are used
    // make the counted wait of the first slot a full one.
    auto step = [&](uint32_t k, uint32_t i, bool refill) {
      const auto acc = consume(buf[k], t0 + i + k);
      __builtin_amdgcn_sched_barrier(0);
      if (refill) buf[k] = load(t0 + i + k + kDepth);
      __builtin_amdgcn_sched_barrier(0);
      fold(acc, t0 + i + k);
      __builtin_amdgcn_sched_barrier(0);
    };
#pragma unroll
    for (uint32_t k = 0; k < kDepth; ++k) {
      buf[k] = load(t0 + k);
      __builtin_amdgcn_sched_barrier(0);
    }
    // Steady state: every step issues one load. The first group stands in
    // front of the loop so that the loop is entered with the same loads
    // and stores in flight as its back edge brings, and its waits count
    // for the steady state, not for the prologue.
    uint32_t i = 0;
#pragma unroll
    for (uint32_t k = 0; k < kDepth; ++k) step(k, i, true);
    for (i = kDepth; i + 2u * kDepth <= n; i += kDepth) {
#pragma unroll
      for (uint32_t k = 0; k < kDepth; ++k) step(k, i, true);
    }
    // kDepth <= n - i < 2*kDepth tiles left: drain the slots, and the
    // fewer than kDepth tiles behind them go one by one
#pragma unroll
    for (uint32_t k = 0; k < kDepth; ++k) step(k, i, false);
    plain(i + kDepth, n);
  }
}

// What a wave of the walk's warm tail does plainly (digest_walk, kWarm).
constexpr int kWarmNone = 0;
constexpr int kWarmStores = 1;
constexpr int kWarmLoads = 2;

// The batched digest walk over walk_descs: a desc is a whole object at
// object-offset 0 (CopyDesc) or a segment of a striped object (StripeSeg).
// Every tile is loaded once with the MFMA A-fragment lane map (fully
// coalesced) and hashed in registers; leaving a desc costs a 64-lane
// reduction + one atomic. out[i] accumulates desc i's partial sums and is
// finalized by a follow-up kernel.
//   kCopy:     also store the fragment to dst with the same lane map.
//   kDepth:    software pipeline over a run of full tiles — a tile is stored
//              and handed to the MFMA, its slot is refilled with the tile
//              kDepth ahead, then comes the long VALU fold with kDepth loads
//              outstanding. The steady loop waits with a counted vmcnt
//              (2*kDepth-2 loads and stores stay in flight), never for
//              everything. Loads never reach past the run, so nothing is
//              read beyond a desc's last full tile. 0: load, then fold (the
//              walk without the store is VALU-bound).
//   StripeSeg: the tile's group fold feeds two sums — out[i], slots counted
//              from the segment's start, and obj_out[seg.obj], slots counted
//              from the object's start (all 64-bit). A segment at tile 0 of
//              its object has the same slots in both, so it runs one mix per
//              tile and adds its one sum to both accumulators.
//   kNtLoads:  full tiles are loaded nontemporal. The copying kernels do; on
//              the 512 × 1 MiB put it is worth 3–5 % of the launch
//              (profiles/walk_persistent_checks.md). The hash-only walk was
//              not measured with it and loads plainly.
//   kWarm:     the walk has a warm tail, the global tiles from warm_begin on
//              (>= total_tiles: none). A wave whose range begins there
//              accesses its full tiles plainly, so that they allocate in the
//              Infinity Cache: its stores with kWarmStores, its loads with
//              kWarmLoads. The `nt` bit is an instruction modifier, so the
//              run body exists twice behind one scalar branch per run; a
//              boundary inside a wave's range rounds to the wave. Tail tiles
//              keep their byte path. kWarmNone: no such branch, one body.
template <bool kCopy, int kDepth, typename Desc, bool kNtLoads = kCopy,
          int kWarm = kWarmNone>
__device__ __forceinline__ void digest_walk(
    const Desc* __restrict__ descs, const uint64_t* __restrict__ tile_prefix,
    uint32_t nobjs, uint64_t total_tiles, unsigned long long* __restrict__ out,
    unsigned long long* __restrict__ obj_out = nullptr,
    uint64_t warm_begin = ~0ull) {
  constexpr bool kStripe = std::is_same_v<Desc, StripeSeg>;
  const int lane = threadIdx.x & 63;
  uint64_t begin, end;
  if (!wave_tile_range(total_tiles, begin, end)) return;
  [[maybe_unused]] const bool warm = begin >= warm_begin;

  const i32x4 b_frag = load_b_frag(lane);
  const WReg wr = load_w_reg(lane);
  const uint32_t lane_off = lane_tile_offset(lane);

  const uint8_t* src;
  uint8_t* dst;
  uint64_t nbytes;
  [[maybe_unused]] uint64_t first_slot = 0;  // StripeSeg: first_tile * 64
  [[maybe_unused]] uint32_t obj = 0;
  auto enter = [&](const Desc& d) {
    src = wave_uniform(static_cast<const uint8_t*>(d.src));
    dst = wave_uniform(static_cast<uint8_t*>(d.dst));
    nbytes = wave_uniform(d.nbytes);
    if constexpr (kStripe) {
      first_slot = wave_uniform(d.first_tile) * 64;
      obj = wave_uniform(d.obj);
    }
    return nbytes;
  };

  uint64_t h = 0;
  [[maybe_unused]] uint64_t ho = 0;  // StripeSeg: the object-slot sum
  // StripeSeg, leaving a segment after h was reduced: the object's share
  [[maybe_unused]] auto flush_object = [&] {
    if (first_slot != 0) ho = wave_sum_u64(ho);
    else ho = h;
    if (lane == 0 && ho != 0) atomicAdd(&obj_out[obj], ho);
    ho = 0;
  };
  auto leave = [&](uint32_t i) {
    h = wave_sum_u64(h);
    if (lane == 0 && h != 0) atomicAdd(&out[i], h);
    if constexpr (kStripe) flush_object();
    h = 0;
  };
  // tile t of the current desc, projected: the VALU part of its hash
  auto fold = [&](const i32x16& acc, uint64_t t) {
    const uint64_t f = fold_group(acc, wr);
    const uint64_t slot = t * 64 + lane;
    h += mix_slot(f, slot);
    if constexpr (kStripe)
      if (first_slot != 0) ho += mix_slot(f, first_slot + slot);
  };
  // n >= 1 full tiles of the current desc, from its tile t0
  auto full_run = [&](uint64_t t0, uint32_t n) {
    // warm_tag: the run belongs to a wave of the warm tail
    auto body = [&](auto warm_tag) {
      constexpr bool kWarmRun = decltype(warm_tag)::value;
      constexpr bool kNtSt = !(kWarmRun && (kWarm & kWarmStores));
      constexpr bool kNtLd = kNtLoads && !(kWarmRun && (kWarm & kWarmLoads));
      run_tiles<kDepth, i32x4>(
          t0, n,
          [&](uint64_t t) {
            return load_a_frag<kNtLd>(src + t * kTileBytes, lane_off);
          },
          // the fragment's last uses: the store and the MFMA
          [&](const i32x4& a, uint64_t t) {
            if constexpr (kCopy)
              store_a_frag<kNtSt>(dst + t * kTileBytes, lane_off, a);
            return project_tile(a, b_frag);
          },
          fold);
    };
    if constexpr (kWarm != kWarmNone)
      if (warm) return body(std::true_type{});
    body(std::false_type{});
  };
  // zero-padded hash, byte-guarded store
  auto tail_tile = [&](uint64_t t) {
    const uint64_t toff = t * kTileBytes;
    const i32x4 a = load_a_frag_guarded(src, toff, nbytes, lane_off);
    if constexpr (kCopy) store_a_frag_guarded(dst, toff, nbytes, lane_off, a);
    fold(project_tile(a, b_frag), t);
  };
  walk_descs(descs, tile_prefix, nobjs, begin, end, enter, leave, full_run,
             tail_tile);
}

// Tiles per load stream (old and new) that the patch walk keeps in flight:
// 2 × 2 loads, as many as the copying walk's kWalkDepth, on twice the
// fragment registers per tile.
constexpr int kPatchDepth = 2;

// The walk of the in-place range patch (patch.hip) over walk_descs. One run =
// one PatchSeg: new bytes at src that replace the old ones at dst, from a
// tile boundary of the run's shard and of its object. The ranges and the
// boundary loop are the ones digest_walk stands on; what differs is that
// every tile is loaded twice — old from dst, new from src — both fragments
// go through the MFMA and the group fold, and the sums take the DIFFERENCE
// mix_slot(f_new, slot) − mix_slot(f_old, slot) (u64 wraparound):
// shard_acc[run.shard] with slots counted from the shard's start,
// obj_acc[run.obj] with slots counted from the object's start. The host
// seeds both with unfinalize(old digest); nothing is cleared here. A run at
// the same tile of both (a single-shard object, or the first shard) runs one
// pair of mixes and adds it to both.
//
// Ordering: a tile's new bytes go to dst only after the load of its old
// bytes has returned. Per tile the old load is issued BEFORE the new load
// (the scheduling barrier between them keeps it so), vector loads return in
// order, and the store's data is the new fragment — so the wait the store
// needs covers the old load as well. The tail tile's byte accesses wait for
// everything explicitly. Nothing leans on the memory system's order between
// a load and a younger store to one address.
//
// Both loads are nontemporal: the old tile is overwritten at once and the
// new one is not read again (unmeasured against plain loads).
template <int kDepth>
__device__ __forceinline__ void patch_walk(
    const PatchSeg* __restrict__ segs, const uint64_t* __restrict__ tile_prefix,
    uint32_t nseg, uint64_t total_tiles,
    unsigned long long* __restrict__ shard_acc,
    unsigned long long* __restrict__ obj_acc) {
  static_assert(kDepth >= 1);
  const int lane = threadIdx.x & 63;
  uint64_t begin, end;
  if (!wave_tile_range(total_tiles, begin, end)) return;

  const i32x4 b_frag = load_b_frag(lane);
  const WReg wr = load_w_reg(lane);
  const uint32_t lane_off = lane_tile_offset(lane);

  const uint8_t* src;
  uint8_t* dst;
  uint64_t nbytes, shard_slot, obj_slot;
  uint32_t shard, obj;
  auto enter = [&](const PatchSeg& d) {
    src = wave_uniform(static_cast<const uint8_t*>(d.src));
    dst = wave_uniform(static_cast<uint8_t*>(d.dst));
    nbytes = wave_uniform(d.nbytes);
    shard_slot = wave_uniform(d.shard_tile) * 64;
    obj_slot = wave_uniform(d.obj_tile) * 64;
    shard = wave_uniform(d.shard);
    obj = wave_uniform(d.obj);
    return nbytes;
  };

  uint64_t hs = 0, ho = 0;  // the shard-slot and object-slot differences
  // leaving a run: its shares of the two accumulators
  auto leave = [&](uint32_t) {
    hs = wave_sum_u64(hs);
    if (shard_slot != obj_slot) ho = wave_sum_u64(ho);
    else ho = hs;
    if (lane == 0 && hs != 0) atomicAdd(&shard_acc[shard], hs);
    if (lane == 0 && ho != 0) atomicAdd(&obj_acc[obj], ho);
    hs = ho = 0;
  };
  // a tile's old and new bytes: the fragments and their projections
  struct Pair {
    i32x4 o, n;
  };
  struct Acc {
    i32x16 o, n;
  };
  // tile t of the current run, old and new projected
  auto fold = [&](const Acc& acc, uint64_t t) {
    const uint64_t f_old = fold_group(acc.o, wr);
    const uint64_t f_new = fold_group(acc.n, wr);
    const uint64_t slot = t * 64 + lane;
    hs += mix_slot(f_new, shard_slot + slot) - mix_slot(f_old, shard_slot + slot);
    if (shard_slot != obj_slot)
      ho += mix_slot(f_new, obj_slot + slot) - mix_slot(f_old, obj_slot + slot);
  };
  // old first, then new: see "Ordering" above
  auto load_pair = [&](uint64_t tile) {
    Pair p;
    p.o = load_a_frag<true>(dst + tile * kTileBytes, lane_off);
    __builtin_amdgcn_sched_barrier(0);
    p.n = load_a_frag<true>(src + tile * kTileBytes, lane_off);
    __builtin_amdgcn_sched_barrier(0);
    return p;
  };
  // n >= 1 full tiles of the current run, from its tile t0
  auto full_run = [&](uint64_t t0, uint32_t n) {
    run_tiles<kDepth, Pair>(
        t0, n, load_pair,
        [&](const Pair& p, uint64_t t) {
          store_a_frag(dst + t * kTileBytes, lane_off, p.n);
          return Acc{project_tile(p.o, b_frag), project_tile(p.n, b_frag)};
        },
        fold);
  };
  // byte-guarded loads of both, zero-padded; every load has returned before
  // the first byte is stored
  auto tail_tile = [&](uint64_t t) {
    const uint64_t toff = t * kTileBytes;
    const i32x4 a_old = load_a_frag_guarded(dst, toff, nbytes, lane_off);
    const i32x4 a_new = load_a_frag_guarded(src, toff, nbytes, lane_off);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    store_a_frag_guarded(dst, toff, nbytes, lane_off, a_new);
    fold(Acc{project_tile(a_old, b_frag), project_tile(a_new, b_frag)}, t);
  };
  walk_descs(segs, tile_prefix, nseg, begin, end, enter, leave, full_run,
             tail_tile);
}

// One edge tile of a byte-granular patch (patch.hip), one wave: the tile is
// overwritten in part, [lo, hi) of it, and moves its shard's and its object's
// sums by term(composed tile) − term(old tile), into the accumulators the
// patch walk adds to. The old tile is loaded with the byte path (zero past
// valid, nothing read there), the composed fragment takes src's bytes inside
// the window, and only the window is stored — after every load has returned,
// waited for explicitly as in the walk's tail tile, so nothing leans on the
// memory system's order between a load and a younger store to one address.
// check_patch_edges keeps every other wave of the launch, and the run kernel
// before it on the stream, off this tile.
__device__ __forceinline__ void patch_edge_tile(
    const PatchEdge& d, int lane, unsigned long long* __restrict__ shard_acc,
    unsigned long long* __restrict__ obj_acc) {
  const uint8_t* src = wave_uniform(static_cast<const uint8_t*>(d.src));
  uint8_t* tile = wave_uniform(static_cast<uint8_t*>(d.tile));
  const uint32_t lo = wave_uniform(d.lo);
  const uint32_t hi = wave_uniform(d.hi);
  const uint32_t valid = wave_uniform(d.valid);
  const uint64_t shard_slot = wave_uniform(d.shard_tile) * 64;
  const uint64_t obj_slot = wave_uniform(d.obj_tile) * 64;
  const uint32_t shard = wave_uniform(d.shard);
  const uint32_t obj = wave_uniform(d.obj);

  const i32x4 b_frag = load_b_frag(lane);
  const WReg wr = load_w_reg(lane);
  const uint32_t lane_off = lane_tile_offset(lane);

  const i32x4 a_old = load_a_frag_guarded(tile, 0, valid, lane_off);
  const i32x4 a_new = compose_a_frag_windowed(a_old, src, lo, hi, lane_off);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  store_a_frag_windowed(tile, lo, hi, lane_off, a_new);

  const uint64_t f_old = fold_group(project_tile(a_old, b_frag), wr);
  const uint64_t f_new = fold_group(project_tile(a_new, b_frag), wr);
  uint64_t hs = mix_slot(f_new, shard_slot + lane) -
                mix_slot(f_old, shard_slot + lane);
  uint64_t ho = 0;
  if (shard_slot != obj_slot)
    ho = mix_slot(f_new, obj_slot + lane) - mix_slot(f_old, obj_slot + lane);
  hs = wave_sum_u64(hs);
  if (shard_slot != obj_slot) ho = wave_sum_u64(ho);
  else ho = hs;
  if (lane == 0 && hs != 0) atomicAdd(&shard_acc[shard], hs);
  if (lane == 0 && ho != 0) atomicAdd(&obj_acc[obj], ho);
}

}  // namespace blackbird::gpu::dev
