// Host-side rules of the in-place range patch (gpu::fused_patch,
// csrc/hip/patch.hip), the twin of stripe_plan.h: the run descriptor, the
// argument check and the planners that turn a byte range of one copy into
// per-shard pieces. Pure host code, no HIP types — the clients, the bindings
// and the tests use it without a GPU.
//
// bbhash64 is a commutative u64 sum H of per-tile terms, recorded as
// mix64(H ^ nbytes) with mix64 a bijection (digest_spec.h). Overwriting
// whole tiles in place therefore moves a digest by the difference of the
// tiles' terms alone:
//   new = finalize(unfinalize(old, n) + Σ term(new tiles) − Σ term(old tiles), n)
// and only the patched tiles are read. Bytes outside the range are never
// re-hashed, so a corrupt byte there stays detectable after the patch.
#pragma once

#include <algorithm>
#include <cstdint>
#include <optional>
#include <string>
#include <tuple>
#include <vector>

#include "blackbird/common/result.h"
#include "blackbird/gpu/digest_spec.h"
#include "blackbird/gpu/stripe_plan.h"

namespace blackbird::gpu {

// One contiguous run of new bytes, written over the old ones at dst.
struct PatchSeg {
  const void* src;      // the new bytes
  void* dst;            // the run's first byte in the pool
  uint64_t nbytes;
  uint64_t shard_tile;  // the run's first 1 KiB tile, counted in its SHARD
  uint64_t obj_tile;    // ... and counted in its OBJECT
  uint32_t shard;       // index into the shard arrays
  uint32_t obj;         // index into the object arrays
};

// The two halves of check_patch_segs. A one-shot launch knows both at once;
// a replayed step (FusedPatchPlan) knows the runs when it is built and the
// old digests only when it runs.
//
// INVALID_ARGUMENT if an old digest is 0, which means "not recorded".
inline Result<void> check_patch_digests(const uint64_t* shard_old,
                                        uint32_t nshard,
                                        const uint64_t* obj_old,
                                        uint32_t nobj) {
  for (uint32_t i = 0; i < nshard; ++i)
    if (shard_old[i] == 0)
      return Error{ErrorCode::INVALID_ARGUMENT,
                   "patch shard " + std::to_string(i) + ": no recorded digest"};
  for (uint32_t i = 0; i < nobj; ++i)
    if (obj_old[i] == 0)
      return Error{ErrorCode::INVALID_ARGUMENT,
                   "patch object " + std::to_string(i) + ": no recorded digest"};
  return {};
}

// INVALID_ARGUMENT unless: every index is in range; every run lies inside
// its shard and its object and covers whole tiles of both — only a run that
// ends exactly at its object's end, which must be its shard's end too, may
// end mid-tile (only there does the spec zero-pad); src and dst are 16-byte
// aligned and [src, src+n) does not overlap [dst, dst+n); and no two runs
// cover the same tile of the same shard (the bytes left behind and the old
// terms subtracted would depend on wave order). Zero-length runs are legal.
inline Result<void> check_patch_geometry(const PatchSeg* segs, uint32_t nseg,
                                         const uint64_t* shard_lens,
                                         uint32_t nshard,
                                         const uint64_t* obj_sizes,
                                         uint32_t nobj) {
  using digest::kTileBytes;
  auto bad = [](uint32_t i, const char* what) {
    return Error{ErrorCode::INVALID_ARGUMENT,
                 "patch run " + std::to_string(i) + ": " + what};
  };
  // (shard, first tile, tile count, run) of the non-empty runs
  std::vector<std::tuple<uint32_t, uint64_t, uint64_t, uint32_t>> cover;
  for (uint32_t i = 0; i < nseg; ++i) {
    const PatchSeg& s = segs[i];
    if (s.shard >= nshard) return bad(i, "shard index out of range");
    if (s.obj >= nobj) return bad(i, "object index out of range");
    const uint64_t slen = shard_lens[s.shard];
    const uint64_t size = obj_sizes[s.obj];
    // tile*1024 + nbytes <= length, without overflow
    if (s.shard_tile > slen / kTileBytes) return bad(i, "starts past its shard");
    if (s.obj_tile > size / kTileBytes) return bad(i, "starts past its object");
    const uint64_t sbegin = s.shard_tile * kTileBytes;
    const uint64_t obegin = s.obj_tile * kTileBytes;
    if (s.nbytes > slen - sbegin) return bad(i, "runs past its shard");
    if (s.nbytes > size - obegin) return bad(i, "runs past its object");
    if (s.nbytes % kTileBytes != 0 &&
        (obegin + s.nbytes != size || sbegin + s.nbytes != slen))
      return bad(i, "partial tile inside its object");
    if (s.nbytes == 0) continue;
    const uint64_t a = reinterpret_cast<uint64_t>(s.src);
    const uint64_t b = reinterpret_cast<uint64_t>(s.dst);
    if (a % 16 != 0 || b % 16 != 0) return bad(i, "address not 16-byte aligned");
    if (s.nbytes > ~a || s.nbytes > ~b) return bad(i, "address range wraps");
    if (a < b + s.nbytes && b < a + s.nbytes)
      return bad(i, "source overlaps destination");
    cover.emplace_back(s.shard, s.shard_tile,
                       (s.nbytes + kTileBytes - 1) / kTileBytes, i);
  }
  std::sort(cover.begin(), cover.end());
  for (size_t k = 1; k < cover.size(); ++k) {
    const auto& [ps, pt, pn, pi] = cover[k - 1];
    const auto& [cs, ct, cn, ci] = cover[k];
    if (ps == cs && ct < pt + pn) return bad(ci, "covers a tile of another run");
  }
  return {};
}

// Both: the digests first, then the runs.
inline Result<void> check_patch_segs(const PatchSeg* segs, uint32_t nseg,
                                     const uint64_t* shard_lens,
                                     const uint64_t* shard_old, uint32_t nshard,
                                     const uint64_t* obj_sizes,
                                     const uint64_t* obj_old, uint32_t nobj) {
  BB_RETURN_IF_ERROR(check_patch_digests(shard_old, nshard, obj_old, nobj));
  return check_patch_geometry(segs, nseg, shard_lens, nshard, obj_sizes, nobj);
}

// What a byte range touches of one shard of a copy.
struct RangePiece {
  uint32_t shard;      // index into the copy's shards
  uint64_t shard_off;  // byte offset in the shard
  uint64_t obj_off;    // byte offset in the object
  uint64_t nbytes;
};

// The pieces of [offset, offset+length) of a copy whose shards hold the
// object's bytes back to back, in shard order; any offset and length inside
// the object (what a ranged get needs). nullopt: the lengths do not add up
// to the object, or the range leaves it. An empty range has no piece.
inline std::optional<std::vector<RangePiece>> range_pieces(
    uint64_t obj_size, const std::vector<uint64_t>& shard_lens, uint64_t offset,
    uint64_t length) {
  if (offset > obj_size || length > obj_size - offset) return std::nullopt;
  std::vector<RangePiece> out;
  const uint64_t end = offset + length;
  uint64_t off = 0;
  for (size_t i = 0; i < shard_lens.size(); ++i) {
    const uint64_t len = shard_lens[i];
    if (len > obj_size - off) return std::nullopt;
    const uint64_t lo = std::max(off, offset);
    const uint64_t hi = std::min(off + len, end);
    if (lo < hi)
      out.push_back({static_cast<uint32_t>(i), lo - off, lo, hi - lo});
    off += len;
  }
  if (off != obj_size) return std::nullopt;
  return out;
}

// The same for an in-place patch: every piece is a legal PatchSeg once it has
// addresses (shard_tile = shard_off / 1024, obj_tile = obj_off / 1024).
// nullopt ("rewrite the object instead"): plan_stripe refuses the copy, the
// offset is not a multiple of 1024, or the length is not and the range does
// not end at the object's end.
inline std::optional<std::vector<RangePiece>> plan_patch(
    uint64_t obj_size, const std::vector<uint64_t>& shard_lens, uint64_t offset,
    uint64_t length) {
  using digest::kTileBytes;
  if (!plan_stripe(obj_size, shard_lens)) return std::nullopt;
  if (offset % kTileBytes != 0) return std::nullopt;
  if (offset > obj_size || length > obj_size - offset) return std::nullopt;
  if (length % kTileBytes != 0 && offset + length != obj_size)
    return std::nullopt;
  return range_pieces(obj_size, shard_lens, offset, length);
}

// ------------------------------------------------ byte-granular patches
// A tile's term depends only on its 1024 bytes and its slot, so a tile that is
// overwritten IN PART moves a digest by term(composed tile) − term(old tile),
// the composed tile being the old bytes outside [lo, hi) and the new bytes
// inside. Such a tile is an EDGE of a byte range: at most one at its head and
// one at its tail, with whole-tile runs (PatchSegs) between them.

// One edge tile. Its bytes go one by one: no alignment is asked of src or
// tile.
struct PatchEdge {
  const void* src;      // the first NEW byte of this tile
  void* tile;           // the tile's first byte in the pool
  uint32_t lo, hi;      // the new bytes take [lo, hi) of the tile, lo < hi <= valid
  uint32_t valid;       // bytes of the tile that exist: 1024, less only in the
                        // last tile of the object (which is its shard's last too)
  uint64_t shard_tile, obj_tile;  // the tile, counted in its shard / its object
  uint32_t shard, obj;            // indices into the shard / object arrays
};
static_assert(sizeof(PatchEdge) % 8 == 0);

// INVALID_ARGUMENT unless, for every edge: the indices are in range; the tile
// exists in its shard and in its object and valid is what both leave of it
// (min(1024, length − tile·1024), the same counted either way);
// lo < hi <= valid; [src, src+hi−lo) does not overlap [tile, tile+valid); and
// no run and no other edge of the same shard covers the tile (wave order
// would decide which old term is subtracted). The runs must have passed
// check_patch_geometry.
inline Result<void> check_patch_edges(const PatchEdge* edges, uint32_t nedge,
                                      const PatchSeg* segs, uint32_t nseg,
                                      const uint64_t* shard_lens,
                                      uint32_t nshard,
                                      const uint64_t* obj_sizes,
                                      uint32_t nobj) {
  using digest::kTileBytes;
  if (nedge == 0) return {};
  auto bad = [](uint32_t i, const char* what) {
    return Error{ErrorCode::INVALID_ARGUMENT,
                 "patch edge " + std::to_string(i) + ": " + what};
  };
  // (shard, first tile, tile count) of the non-empty runs and of the edges
  std::vector<std::tuple<uint32_t, uint64_t, uint64_t>> runs, tiles;
  for (uint32_t i = 0; i < nseg; ++i)
    if (segs[i].nbytes != 0)
      runs.emplace_back(segs[i].shard, segs[i].shard_tile,
                        (segs[i].nbytes + kTileBytes - 1) / kTileBytes);
  std::sort(runs.begin(), runs.end());
  // bytes of tile t that exist in `len` bytes; 0: the tile does not
  auto left = [](uint64_t len, uint64_t t) -> uint64_t {
    if (t > len / kTileBytes) return 0;
    return std::min<uint64_t>(kTileBytes, len - t * kTileBytes);
  };
  for (uint32_t i = 0; i < nedge; ++i) {
    const PatchEdge& e = edges[i];
    if (e.shard >= nshard) return bad(i, "shard index out of range");
    if (e.obj >= nobj) return bad(i, "object index out of range");
    const uint64_t in_shard = left(shard_lens[e.shard], e.shard_tile);
    const uint64_t in_obj = left(obj_sizes[e.obj], e.obj_tile);
    if (in_shard == 0) return bad(i, "tile past its shard");
    if (in_obj == 0) return bad(i, "tile past its object");
    if (e.valid != in_shard || e.valid != in_obj)
      return bad(i, "valid is not what its shard and object leave of the tile");
    if (e.lo >= e.hi || e.hi > e.valid) return bad(i, "not lo < hi <= valid");
    const uint64_t a = reinterpret_cast<uint64_t>(e.src);
    const uint64_t b = reinterpret_cast<uint64_t>(e.tile);
    const uint64_t n = e.hi - e.lo;
    if (n > ~a || e.valid > ~b) return bad(i, "address range wraps");
    if (a < b + e.valid && b < a + n) return bad(i, "source overlaps its tile");
    // the last run that starts at or before the tile
    auto it = std::upper_bound(
        runs.begin(), runs.end(),
        std::make_tuple(e.shard, e.shard_tile, ~uint64_t{0}));
    if (it != runs.begin()) {
      const auto& [rs, rt, rn] = *(it - 1);
      if (rs == e.shard && e.shard_tile < rt + rn)
        return bad(i, "lies on a tile of a run");
    }
    tiles.emplace_back(e.shard, e.shard_tile, i);
  }
  std::sort(tiles.begin(), tiles.end());
  for (size_t k = 1; k < tiles.size(); ++k)
    if (std::get<0>(tiles[k - 1]) == std::get<0>(tiles[k]) &&
        std::get<1>(tiles[k - 1]) == std::get<1>(tiles[k]))
      return bad(static_cast<uint32_t>(std::get<2>(tiles[k])),
                 "lies on the tile of another edge");
  return {};
}

// An edge before it has addresses.
struct EdgePiece {
  uint32_t shard;       // index into the copy's shards
  uint64_t shard_tile;  // the tile, counted in the shard
  uint64_t obj_tile;    // ... and in the object
  uint32_t lo, hi, valid;
  uint64_t src_off;     // where the tile's new bytes begin in the caller's
};

struct BytePatchPlan {
  std::vector<RangePiece> runs;  // whole tiles (or to the object's end)
  std::vector<EdgePiece> edges;
};

// plan_patch at byte granularity: [offset, offset+length) of one copy as
// whole-tile runs, each a legal PatchSeg once it has addresses, plus the edge
// tiles at the range's head and tail. Shards start on tile boundaries of their
// object, so only the first piece can have a head edge and only the last a
// tail edge: at most two edges. A range that ends at the object's end ends in
// a run (the tail path the runs have), not in an edge, unless it also starts
// inside that tile. For every range plan_patch accepts this is plan_patch's
// pieces and no edge. nullopt: plan_stripe refuses the copy, or the range
// leaves the object.
inline std::optional<BytePatchPlan> plan_patch_bytes(
    uint64_t obj_size, const std::vector<uint64_t>& shard_lens, uint64_t offset,
    uint64_t length) {
  using digest::kTileBytes;
  if (!plan_stripe(obj_size, shard_lens)) return std::nullopt;
  auto pieces = range_pieces(obj_size, shard_lens, offset, length);
  if (!pieces) return std::nullopt;
  BytePatchPlan out;
  for (const RangePiece& p : *pieces) {
    const uint64_t slen = shard_lens[p.shard];
    const uint64_t shard_base = p.obj_off - p.shard_off;  // a tile boundary
    uint64_t a = p.shard_off;
    const uint64_t e = p.shard_off + p.nbytes;
    auto edge = [&](uint64_t from, uint64_t to) {  // inside one tile
      const uint64_t t = from / kTileBytes;
      out.edges.push_back(
          {p.shard, t, (shard_base + from) / kTileBytes,
           static_cast<uint32_t>(from - t * kTileBytes),
           static_cast<uint32_t>(to - t * kTileBytes),
           static_cast<uint32_t>(std::min(kTileBytes, slen - t * kTileBytes)),
           shard_base + from - offset});
    };
    if (a % kTileBytes != 0) {  // head
      const uint64_t stop =
          std::min(e, (a / kTileBytes + 1) * uint64_t{kTileBytes});
      edge(a, stop);
      a = stop;
    }
    if (a == e) continue;
    const bool to_end = shard_base + e == obj_size;
    const uint64_t run_end = to_end ? e : e - e % kTileBytes;
    if (a < run_end)
      out.runs.push_back({p.shard, a, shard_base + a, run_end - a});
    if (run_end < e) edge(run_end, e);  // tail
  }
  return out;
}

}  // namespace blackbird::gpu
