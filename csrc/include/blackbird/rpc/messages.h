// Request and response bodies that both ends of an RPC declare: one
// definition, so the sender and the receiver cannot drift apart. A message
// only one side names, or whose two sides differ on purpose (the client's
// encode-only write requests), stays in its translation unit.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "blackbird/common/serde.h"
#include "blackbird/common/types.h"

namespace blackbird {

// ---- keystone ⇄ client ----
struct KeyMsg {
  std::string key;
  BB_FIELDS(key)
};
struct KeysMsg {
  std::vector<std::string> keys;
  BB_FIELDS(keys)
};
struct BoolMsg {
  uint8_t v = 0;
  BB_FIELDS(v)
};
struct U64Msg {  // also the worker's DATA_CHECKSUM answer
  uint64_t v = 0;
  BB_FIELDS(v)
};
struct StatusListMsg {
  std::vector<int32_t> statuses;
  BB_FIELDS(statuses)
};
struct WorkersInfoMsg {
  std::vector<WorkerInfo> workers;
  BB_FIELDS(workers)
};
struct PoolsMsg {
  std::vector<MemoryPool> pools;
  BB_FIELDS(pools)
};
struct PutCompleteListMsg {
  std::vector<PutCompleteRequest> reqs;
  BB_FIELDS(reqs)
};

// ---- worker data plane ⇄ client, keystone, peer workers ----
struct ReadReq {
  std::string pool_id;
  uint64_t offset = 0;
  uint64_t length = 0;
  BB_FIELDS(pool_id, offset, length)
};
struct ChecksumReq {
  std::string pool_id;
  uint64_t offset = 0;
  uint64_t length = 0;
  BB_FIELDS(pool_id, offset, length)
};
// DATA_PULL: fill [dst_offset, dst_offset + total_len) of dst_pool from the
// ordered source shards
struct PullReq {
  std::string dst_pool;
  uint64_t dst_offset = 0;
  uint64_t total_len = 0;
  std::vector<ShardPlacement> srcs;
  BB_FIELDS(dst_pool, dst_offset, total_len, srcs)
};

}  // namespace blackbird
