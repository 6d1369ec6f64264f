// Wire codec of the compact v2 batch protocol: BATCH_PUT_START2,
// BATCH_GET_WORKERS2, BATCH_UPSERT_START and BATCH_COMMIT_TOKEN, and of the
// two session messages that serve striped copies, BATCH_SESSION_OPEN and
// BATCH_COMMIT_TOKEN_SHARDS, and of the patch session's start,
// BATCH_PATCH_START_TOKEN. Clients and the keystone handlers both go
// through these functions; nothing else spells the layouts out.
//
//   BATCH_PUT_START2 request
//     u32 count | u64 uniform_size (0 = per-item sizes follow) |
//     [u64 size]*count | str key * count | PlacementConfig | [u8 want_token]
//   BATCH_PUT_START2 response
//     u64 view_version | u64 token (0 = none) | pool table | count items:
//       u8 0, u8 ncopies, {u16 pool_idx, u64 offset}*ncopies   or
//       u8 1, i32 status
//   BATCH_GET_WORKERS2 request
//     u32 count | str key * count
//   BATCH_GET_WORKERS2 response
//     pool table | count items:
//       u8 0, u64 size, u64 checksum, u8 ncopies, {u16, u64}*ncopies   or
//       u8 1, i32 status   (NOT_IMPLEMENTED = striped object: use v1)
//   BATCH_UPSERT_START   u64 token
//   BATCH_COMMIT_TOKEN   u64 token | u8 flags (bit 0: release) | u32 n | u64*n
//   BATCH_SESSION_OPEN request
//     u32 count | {str key, u64 size}*count | u8 flags (bit 0: allow striped)
//   BATCH_SESSION_OPEN response
//     u64 token (0 = refused)
//   BATCH_COMMIT_TOKEN_SHARDS
//     u64 token | u8 flags (bit 0: release) | u32 n | u64*n | u32 m | u64*m
//     (n object digests; m shard digests in object, copy, shard order)
//   BATCH_PATCH_START_TOKEN request
//     u64 token
//   BATCH_PATCH_START_TOKEN response
//     u32 n | u64*n | u32 m | u64*m
//     (the recorded digests, in the order BATCH_COMMIT_TOKEN_SHARDS takes the
//     new ones: n object checksums; m shard digests)
//   pool table           u16 npools | str pool_id * npools
//
// The responses carry no item count (the caller knows how many it asked for).
#pragma once

#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "blackbird/common/result.h"
#include "blackbird/common/serde.h"
#include "blackbird/common/types.h"

namespace blackbird::wire {

struct Place {
  uint16_t pool_idx = 0;  // index into BatchPlacements::pools — NOT range
                          // checked by the decoder: each caller has its own
                          // policy for pool_idx >= pools.size()
  uint64_t offset = 0;
};

struct ItemPlaces {
  int32_t status = 0;        // != 0: no places
  uint32_t first_place = 0;  // places[first_place .. first_place + ncopies)
  uint8_t ncopies = 0;
  uint64_t size = 0;      // get response only
  uint64_t checksum = 0;  // get response only
};

// Both responses, decoded flat: one places array for the whole batch.
struct BatchPlacements {
  uint64_t view_version = 0;  // put response only
  uint64_t token = 0;         // put response only
  std::vector<PoolId> pools;
  std::vector<ItemPlaces> items;
  std::vector<Place> places;

  const Place* places_of(const ItemPlaces& it) const {
    return places.data() + it.first_place;
  }
};

struct PutStart2Request {
  std::vector<ObjectKey> keys;
  std::vector<uint64_t> sizes;
  PlacementConfig cfg;
  uint8_t want_token = 0;  // absent on the wire (older clients) = 0
};

struct CommitToken {
  uint64_t token = 0;
  uint8_t flags = 0;  // bit 0: release the session after the commit
  std::vector<uint64_t> digests;
};

struct SessionOpen {
  std::vector<ObjectKey> keys;
  std::vector<uint64_t> sizes;
  uint8_t flags = 0;  // bit 0: striped copies may join
};

struct CommitTokenShards {
  uint64_t token = 0;
  uint8_t flags = 0;  // bit 0: release the session after the commit
  std::vector<uint64_t> obj_digests;
  std::vector<uint64_t> shard_digests;  // object, copy, shard order
};

// What the keystone holds for a patch session's objects when a step starts.
struct PatchStartDigests {
  std::vector<uint64_t> obj_digests;
  std::vector<uint64_t> shard_digests;  // object, copy, shard order
};

// ---- requests (clients encode; items are keys or structs with .key/.size)
template <typename T>
const ObjectKey& key_of(const T& item) {
  if constexpr (std::is_same_v<T, ObjectKey>) return item;
  else return item.key;
}

template <typename Item>
std::string encode_put_start2_request(const std::vector<Item>& items,
                                      const PlacementConfig& cfg,
                                      bool want_token) {
  serde::Enc e;
  e.num<uint32_t>(static_cast<uint32_t>(items.size()));
  // uniform size when possible (the common batched pattern)
  uint64_t uniform = items.empty() ? 1 : items[0].size;
  for (auto& it : items)
    if (it.size != uniform) { uniform = 0; break; }
  e.num<uint64_t>(uniform);
  if (uniform == 0)
    for (auto& it : items) e.num<uint64_t>(it.size);
  for (auto& it : items) e.str(it.key);
  serde::put(e, cfg);
  e.num<uint8_t>(want_token ? 1 : 0);
  return std::move(e.buf);
}

template <typename Item>
std::string encode_get_workers2_request(const std::vector<Item>& items) {
  serde::Enc e;
  e.num<uint32_t>(static_cast<uint32_t>(items.size()));
  for (auto& it : items) e.str(key_of(it));
  return std::move(e.buf);
}

std::string encode_upsert_start(uint64_t token);
// digests[0], digests[stride], ... — n of them (replicated sessions keep one
// digest per copy and commit copy 0's)
std::string encode_commit_token(uint64_t token, bool release,
                                const uint64_t* digests, size_t n,
                                size_t stride = 1);

template <typename Item>
std::string encode_session_open(const std::vector<Item>& items,
                                bool allow_striped) {
  serde::Enc e;
  e.num<uint32_t>(static_cast<uint32_t>(items.size()));
  for (auto& it : items) {
    e.str(it.key);
    e.num<uint64_t>(it.size);
  }
  e.num<uint8_t>(allow_striped ? 1 : 0);
  return std::move(e.buf);
}
std::string encode_session_open_response(uint64_t token);
std::string encode_commit_token_shards(uint64_t token, bool release,
                                       const uint64_t* obj_digests, size_t n,
                                       const uint64_t* shard_digests, size_t m);
std::string encode_patch_start_token(uint64_t token);
std::string encode_patch_start_token_response(const PatchStartDigests& r);

// ---- requests (keystone decodes); PROTOCOL_ERROR on a malformed body
Result<PutStart2Request> decode_put_start2_request(const std::string& body);
Result<std::vector<ObjectKey>> decode_get_workers2_request(
    const std::string& body);
Result<uint64_t> decode_upsert_start(const std::string& body);
Result<CommitToken> decode_commit_token(const std::string& body);
Result<SessionOpen> decode_session_open(const std::string& body);
Result<uint64_t> decode_session_open_response(const std::string& body);
Result<CommitTokenShards> decode_commit_token_shards(const std::string& body);
Result<uint64_t> decode_patch_start_token(const std::string& body);
Result<PatchStartDigests> decode_patch_start_token_response(
    const std::string& body);

// ---- responses
// Pool table under construction: interns pool ids in first-seen order.
class PoolTable {
 public:
  explicit PoolTable(std::vector<PoolId>& names) : names_(names) {}
  uint16_t intern(const PoolId& id) {
    auto [it, fresh] = idx_.emplace(id, static_cast<uint16_t>(names_.size()));
    if (fresh) names_.push_back(id);
    return it->second;
  }

 private:
  std::vector<PoolId>& names_;
  std::map<PoolId, uint16_t> idx_;
};
// Append one item: every shard's pool joins the table; with status 0 the
// first shard of each copy becomes a place.
void append_item(BatchPlacements& out, PoolTable& table, int32_t status,
                 const std::vector<CopyPlacement>& copies, uint64_t size = 0,
                 uint64_t checksum = 0);

std::string encode_put_start2_response(const BatchPlacements& p);
std::string encode_get_workers2_response(const BatchPlacements& p);
// `out` is overwritten (its vectors keep their capacity, so a caller that
// reuses one decodes without allocating); PROTOCOL_ERROR on a short body.
Result<void> decode_put_start2_response(const std::string& body, size_t nitems,
                                        BatchPlacements& out);
Result<void> decode_get_workers2_response(const std::string& body,
                                          size_t nitems, BatchPlacements& out);

}  // namespace blackbird::wire
