// Host-side rules of the fused striped copy+digest launch (gpu::fused_stripe,
// csrc/hip/stripe.hip): the segment descriptor, the argument check and the
// planner that turns one copy's shard lengths into segments. Pure host code,
// no HIP types — the client, the bindings and the tests use it without a GPU.
#pragma once

#include <cstdint>
#include <optional>
#include <string>
#include <vector>

#include "blackbird/common/result.h"
#include "blackbird/gpu/digest_spec.h"

namespace blackbird::gpu {

// One contiguous run of an object's bytes, copied src→dst and hashed. A put
// scatters slices of one buffer to shard addresses, a get gathers shard
// addresses into slices of one buffer; the kernel does not tell them apart.
struct StripeSeg {
  const void* src;
  void* dst;
  uint64_t nbytes;
  uint64_t first_tile;  // the segment's first 1 KiB tile, counted in the OBJECT
  uint32_t obj;         // index into the object arrays
};

// INVALID_ARGUMENT unless every segment names an object, lies inside it,
// starts on a tile of it (by construction: first_tile) and covers whole
// tiles — only a segment that ends exactly at its object's end may end
// mid-tile, because only there does the spec zero-pad. Zero-length segments
// are legal.
inline Result<void> check_stripe_segs(const StripeSeg* segs, uint32_t nseg,
                                      const uint64_t* obj_sizes, uint32_t nobj) {
  using digest::kTileBytes;
  auto bad = [](uint32_t i, const char* what) {
    return Error{ErrorCode::INVALID_ARGUMENT,
                 "stripe segment " + std::to_string(i) + ": " + what};
  };
  for (uint32_t i = 0; i < nseg; ++i) {
    const StripeSeg& s = segs[i];
    if (s.obj >= nobj) return bad(i, "object index out of range");
    const uint64_t size = obj_sizes[s.obj];
    // first_tile*1024 + nbytes <= size, without overflow
    if (s.first_tile > size / kTileBytes) return bad(i, "starts past its object");
    const uint64_t begin = s.first_tile * kTileBytes;
    if (s.nbytes > size - begin) return bad(i, "runs past its object");
    if (s.nbytes % kTileBytes != 0 && begin + s.nbytes != size)
      return bad(i, "partial tile inside its object");
  }
  return {};
}

// A segment before it has addresses: where it sits in the object.
struct StripePiece {
  uint64_t offset;      // byte offset in the object
  uint64_t nbytes;
  uint64_t first_tile;  // offset / 1024
};

// The segments of one copy whose shards hold the object's bytes back to
// back. nullopt ("not fusable"): a shard other than the last is not a whole
// number of tiles, so the next one would not start on a tile boundary — or
// the lengths do not add up to the object.
inline std::optional<std::vector<StripePiece>> plan_stripe(
    uint64_t obj_size, const std::vector<uint64_t>& shard_lens) {
  using digest::kTileBytes;
  std::vector<StripePiece> out;
  out.reserve(shard_lens.size());
  uint64_t off = 0;
  for (size_t i = 0; i < shard_lens.size(); ++i) {
    const uint64_t len = shard_lens[i];
    if (len > obj_size - off) return std::nullopt;
    if (i + 1 < shard_lens.size() && len % kTileBytes != 0) return std::nullopt;
    out.push_back({off, len, off / kTileBytes});
    off += len;
  }
  if (off != obj_size) return std::nullopt;
  return out;
}

}  // namespace blackbird::gpu
