#include "blackbird/client/client.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <future>
#include <thread>

#include <hip/hip_runtime_api.h>

#include "blackbird/client/batch_util.h"
#include "blackbird/client/batch_wire.h"
#include "blackbird/client/pool_mapper.h"
#include "blackbird/common/hex.h"
#include "blackbird/coord/coord.h"
#include "blackbird/common/log.h"
#include "blackbird/gpu/gpu_kernels.h"
#include "blackbird/rpc/messages.h"
#include "blackbird/rpc/methods.h"
#include "blackbird/worker/storage_backend.h"

namespace blackbird {

namespace M = rpc::methods;

namespace {
// encode-only twin of the WriteReq in worker_service.cpp: the payload is
// written straight from the caller's buffer
struct WriteReq {
  std::string pool_id;
  uint64_t offset = 0;
  const void* src = nullptr;  // encode-only
  uint64_t len = 0;
  void enc(serde::Enc& e) const {
    e.str(pool_id);
    e.num(offset);
    e.bytes(src, len);
  }
  void dec(serde::Dec&) {}
};
struct BatchWriteEnc {  // encodes to the worker's BatchWriteReq wire format
  std::vector<WriteReq> writes;
  void enc(serde::Enc& e) const {
    e.num<uint32_t>(static_cast<uint32_t>(writes.size()));
    for (const auto& w : writes) w.enc(e);
  }
  void dec(serde::Dec&) {}
};
struct BatchReadEnc {
  std::vector<ReadReq> reads;
  BB_FIELDS(reads)
};
}  // namespace

// -------------------------------------------------------------- Client

Client::Client(ClientOptions opts)
    : opts_(std::move(opts)), mapper_(std::make_shared<PoolMapper>()) {}

Client::~Client() { close(); }

Result<void> Client::connect() {
  if (opts_.keystone_endpoint.empty()) {
    if (opts_.coord_endpoint.empty())
      return Error{ErrorCode::ENDPOINT_INVALID,
                   "need keystone_endpoint or coord_endpoint"};
    // bootstrap from the coordination service registry (HA: whichever
    // keystone holds the lease re-registers under this prefix, so a fresh
    // connect always finds the current leader)
    coord::CoordClient cc;
    BB_RETURN_IF_ERROR(cc.connect(opts_.coord_endpoint));
    auto reg = cc.get_prefix("/blackbird/services/blackbird-keystone/");
    // with HA pairs, prefer the instance holding the election lease — the
    // registry lists standbys too
    auto leader = cc.get("/blackbird/clusters/" + opts_.cluster_id + "/leader");
    cc.close();
    if (!reg.ok()) return reg.error();
    if (reg.value().empty())
      return Error{ErrorCode::COORD_UNAVAILABLE,
                   "no keystone registered in coordination"};
    opts_.keystone_endpoint = reg.value()[0].value;
    if (leader.ok()) {
      for (const auto& kv : reg.value()) {
        if (kv.key.size() >= leader.value().size() &&
            kv.key.compare(kv.key.size() - leader.value().size(),
                           leader.value().size(), leader.value()) == 0) {
          opts_.keystone_endpoint = kv.value;
          break;
        }
      }
    }
  }
  return meta_.connect(opts_.keystone_endpoint);
}

Result<std::string> Client::meta_call_raw(uint16_t m, const std::string& body,
                                          int timeout_ms) {
  if (timeout_ms <= 0) timeout_ms = opts_.rpc_timeout_ms;
  auto r = meta_.call_raw(m, body, timeout_ms);
  // ~6 s total budget: leader election + registry TTL convergence after an
  // unclean leader death take a few seconds
  for (int attempt = 0; attempt < 20 && !r.ok(); ++attempt) {
    const bool standby = r.code() == ErrorCode::NOT_LEADER;
    switch (r.code()) {
      case ErrorCode::NOT_LEADER:
      case ErrorCode::NOT_CONNECTED:
      case ErrorCode::CONNECT_FAILED:
      case ErrorCode::CONNECTION_CLOSED:
      case ErrorCode::SEND_FAILED:
      case ErrorCode::RECV_FAILED:
        break;
      default:
        return r;  // not a failover condition
    }
    // a standby answer with no discovery path configured cannot improve
    if (standby && opts_.coord_endpoint.empty()) return r;
    std::this_thread::sleep_for(std::chrono::milliseconds(
        std::min(50 * (attempt + 1), standby ? 500 : 400)));
    {
      std::lock_guard<std::mutex> g(reconnect_mu_);
      if (standby || !meta_.connected()) {
        if (!opts_.coord_endpoint.empty())
          opts_.keystone_endpoint.clear();  // force re-discovery
        auto rc = connect();
        if (!rc.ok()) {
          // a dead (or not-yet-elected) leader: keep re-discovering — the
          // registry TTL drops the dead instance and the standby registers
          if (!opts_.coord_endpoint.empty()) opts_.keystone_endpoint.clear();
          continue;
        }
        reconnect_gen_.fetch_add(1);
      }
    }
    r = meta_.call_raw(m, body, timeout_ms);
  }
  return r;
}

void Client::close() {
  meta_.close();
  std::lock_guard<std::mutex> g(data_mu_);
  data_clients_.clear();
}

rpc::RpcClient* Client::data_client(const std::string& endpoint) {
  std::lock_guard<std::mutex> g(data_mu_);
  auto it = data_clients_.find(endpoint);
  if (it != data_clients_.end()) return it->second.get();
  auto c = std::make_unique<rpc::RpcClient>();
  if (!c->connect(endpoint).ok()) return nullptr;
  return data_clients_.emplace(endpoint, std::move(c)).first->second.get();
}

Result<AccessInfo> Client::pool_access(const PoolId& id) {
  {
    std::lock_guard<std::mutex> g(pool_cache_mu_);
    auto it = pool_cache_.find(id);
    if (it != pool_cache_.end()) return it->second;
  }
  auto pools = memory_pools();
  if (!pools.ok()) return pools.error();
  std::lock_guard<std::mutex> g(pool_cache_mu_);
  pool_cache_.clear();
  for (auto& p : pools.value()) pool_cache_[p.pool_id] = p.access;
  auto it = pool_cache_.find(id);
  if (it == pool_cache_.end())
    return Error{ErrorCode::POOL_NOT_FOUND, id};
  return it->second;
}

// ------------------------------------------------------ shard transfer

namespace {
// The direction-specific pieces of move_shard. `pool` is the shard's address
// in a mapped pool, `user` the caller's buffer.
template <bool Write>
using UserPtr = std::conditional_t<Write, const void*, void*>;

template <bool Write>
void host_copy(void* pool, UserPtr<Write> user, uint64_t n) {
  if constexpr (Write) std::memcpy(pool, user, n);
  else std::memcpy(user, pool, n);
}

template <bool Write>
Result<void> device_copy(void* pool, UserPtr<Write> user, uint64_t n) {
  if constexpr (Write)
    return gpu::copy_sync(pool, user, n, hipMemcpyHostToDevice);
  else
    return gpu::copy_sync(user, pool, n, hipMemcpyDeviceToHost);
}

// One-sided copy through a resolved view; only a device copy can fail.
template <bool Write>
Result<void> view_copy(const PoolView& v, const ShardPlacement& s,
                       UserPtr<Write> user) {
  void* pool = v.base + s.offset;
  if (v.device) return device_copy<Write>(pool, user, s.length);
  host_copy<Write>(pool, user, s.length);
  return {};
}

template <bool Write>
Result<void> tcp_copy(rpc::RpcClient& dc, const ShardPlacement& s,
                      UserPtr<Write> user, int timeout_ms) {
  if constexpr (Write) {
    WriteReq req;
    req.pool_id = s.pool_id;
    req.offset = s.offset;
    req.src = user;
    req.len = s.length;
    auto r = dc.call_raw(M::DATA_WRITE, serde::to_bytes(req), timeout_ms);
    if (!r.ok()) return r.error();
  } else {
    ReadReq req{s.pool_id, s.offset, s.length};
    auto r = dc.call_raw(M::DATA_READ, serde::to_bytes(req), timeout_ms);
    if (!r.ok()) return r.error();
    if (r.value().size() != s.length)
      return Error{ErrorCode::SIZE_MISMATCH, "short read"};
    std::memcpy(user, r.value().data(), s.length);
  }
  return {};
}
}  // namespace

template <bool Write>
Result<void> Client::move_shard(const ShardPlacement& s, UserPtr<Write> user) {
  AccessInfo resolved;
  if (s.access.endpoint.empty()) {
    auto r = pool_access(s.pool_id);
    if (!r.ok()) return r.error();
    resolved = std::move(r.value());
  }
  const AccessInfo& a = s.access.endpoint.empty() ? resolved : s.access;
  if (!opts_.force_tcp) {
    PoolView v = PoolMapper::local(s.pool_id);
    if (v.base) {
      // a failed device copy falls on to the later rungs
      if (view_copy<Write>(v, s, user).ok()) return {};
    } else if (v.local) {
      // unmapped same-process pool (direct-IO NVMe tier): call the backend
      // directly instead of framing the bytes through TCP loopback
      if constexpr (Write) return v.local->write(s.offset, user, s.length);
      else return v.local->read(s.offset, user, s.length);
    }
    // one-sided fast path into another process's pool
    v = mapper_->remote(a);
    if (v.base) {
      auto e = view_copy<Write>(v, s, user);
      if (e.ok()) return {};
      BB_LOG(WARN) << "IPC " << (Write ? "write" : "read")
                   << " failed: " << e.error().message
                   << " — falling back to TCP";
    }
  }
  auto* dc = data_client(a.endpoint);
  if (!dc) return Error{ErrorCode::CONNECT_FAILED, "data plane " + a.endpoint};
  return tcp_copy<Write>(*dc, s, user, opts_.rpc_timeout_ms);
}

Result<void> Client::write_shard(const ShardPlacement& s, const void* src) {
  return move_shard<true>(s, src);
}

Result<void> Client::read_shard(const ShardPlacement& s, void* dst) {
  return move_shard<false>(s, dst);
}

namespace {
// Every shard of `copy` with its offset in the object: body(shard, offset)
// runs inline for one shard, on one std::async each for several. Returns the
// per-shard results in shard order, or nullopt, with nothing run, when the
// shard lengths do not add up to `size`.
template <typename Body>
std::optional<std::vector<Result<void>>> walk_copy(const CopyPlacement& copy,
                                                   uint64_t size, Body&& body) {
  uint64_t total = 0;
  for (const auto& s : copy.shards) total += s.length;
  if (total != size) return std::nullopt;
  std::vector<Result<void>> out;
  if (copy.shards.size() == 1) {
    out.push_back(body(copy.shards[0], uint64_t{0}));
    return out;
  }
  std::vector<std::future<Result<void>>> futs;
  uint64_t off = 0;
  for (const auto& s : copy.shards) {
    futs.push_back(std::async(std::launch::async,
                              [&body, &s, off] { return body(s, off); }));
    off += s.length;
  }
  for (auto& f : futs) out.push_back(f.get());
  return out;
}
}  // namespace

Result<void> Client::write_copies(const std::vector<CopyPlacement>& copies,
                                  const void* data, uint64_t size) {
  for (const auto& copy : copies) {
    auto done = walk_copy(copy, size, [&](const ShardPlacement& s, uint64_t off) {
      return write_shard(s, static_cast<const uint8_t*>(data) + off);
    });
    if (!done)
      return Error{ErrorCode::SIZE_MISMATCH, "placement does not cover object"};
    for (auto& r : *done)
      if (!r.ok()) return r.error();
  }
  return {};
}

Result<void> Client::read_copy(const std::vector<CopyPlacement>& copies,
                               void* dst, uint64_t size) {
  Error last{ErrorCode::NO_PLACEMENT, "no copies"};
  for (const auto& copy : copies) {
    auto done = walk_copy(copy, size, [&](const ShardPlacement& s, uint64_t off) {
      return read_shard(s, static_cast<uint8_t*>(dst) + off);
    });
    if (!done) continue;
    bool ok = true;
    for (auto& r : *done)
      if (!r.ok()) {
        ok = false;
        last = r.error();
      }
    if (ok) return {};
  }
  return last;
}

// ------------------------------------------------------------ object ops

namespace {
// Per-copy per-shard standalone digests for striped copies (empty when every
// copy is single-shard — the whole-object checksum covers those). Recorded
// at put time so the scrubber can verify each striped shard independently.
std::vector<std::vector<uint64_t>> host_shard_digests(
    const std::vector<CopyPlacement>& copies, const void* data) {
  bool any_striped = false;
  for (const auto& c : copies)
    if (c.shards.size() > 1) any_striped = true;
  if (!any_striped) return {};
  std::vector<std::vector<uint64_t>> out;
  out.reserve(copies.size());
  for (const auto& c : copies) {
    std::vector<uint64_t> ds;
    uint64_t off = 0;
    for (const auto& s : c.shards) {
      ds.push_back(gpu::checksum_cpu(
          static_cast<const uint8_t*>(data) + off, s.length));
      off += s.length;
    }
    out.push_back(std::move(ds));
  }
  return out;
}
}  // namespace

Result<void> Client::put(const ObjectKey& key, const void* data, uint64_t size,
                         const PlacementConfig& cfg) {
  const uint64_t gen = reconnect_gen_.load();
  auto r = put_once(key, data, size, cfg);
  if (r.ok() || reconnect_gen_.load() == gen ||
      !failover_retriable(static_cast<int32_t>(r.code())))
    return r;
  // leader change mid-put: the new leader never saw the PENDING object —
  // redo once from put_start
  return put_once(key, data, size, cfg);
}

Result<void> Client::put_once(const ObjectKey& key, const void* data,
                              uint64_t size, const PlacementConfig& cfg) {
  PutStartRequest req{key, size, cfg};
  auto start = meta_call<PutStartRequest, PutStartResponse>(M::PUT_START, req,
                                                             opts_.rpc_timeout_ms);
  if (!start.ok()) return start.error();

  auto xfer = write_copies(start->copies, data, size);
  if (!xfer.ok()) {
    meta_call_raw(M::PUT_CANCEL, serde::to_bytes(KeyMsg{key}), opts_.rpc_timeout_ms);
    return xfer.error();
  }
  uint64_t checksum = cfg.checksum ? gpu::checksum_cpu(data, size) : 0;
  PutCompleteRequest done_req{key, checksum, {}};
  if (cfg.checksum)
    done_req.shard_digests = host_shard_digests(start->copies, data);
  auto done = meta_call_raw(M::PUT_COMPLETE, serde::to_bytes(done_req),
                             opts_.rpc_timeout_ms);
  if (!done.ok()) return done.error();
  return {};
}

Result<std::string> Client::get(const ObjectKey& key) {
  auto meta = meta_call<KeyMsg, GetWorkersResponse>(M::GET_WORKERS, KeyMsg{key},
                                                     opts_.rpc_timeout_ms);
  if (!meta.ok()) return meta.error();
  std::string out;
  out.resize(meta->size);
  BB_RETURN_IF_ERROR(read_copy(meta->copies, out.data(), meta->size));
  if (opts_.verify_checksum_on_get && meta->checksum != 0) {
    uint64_t got = gpu::checksum_cpu(out.data(), out.size());
    if (got != meta->checksum)
      return Error{ErrorCode::CHECKSUM_MISMATCH, key};
  }
  return out;
}

Result<uint64_t> Client::get_into(const ObjectKey& key, void* dst,
                                  uint64_t capacity) {
  auto meta = meta_call<KeyMsg, GetWorkersResponse>(M::GET_WORKERS, KeyMsg{key},
                                                     opts_.rpc_timeout_ms);
  if (!meta.ok()) return meta.error();
  if (meta->size > capacity)
    return Error{ErrorCode::SIZE_MISMATCH, "buffer too small"};
  BB_RETURN_IF_ERROR(read_copy(meta->copies, dst, meta->size));
  return meta->size;
}

// ---------------------------------------------------------- ranged access

namespace {
// Whether the tier serves this sub-range as such. The block tiers do IO at
// 4 KiB granularity (an unaligned write there is a read-modify-write of its
// edge blocks), so a piece that is not made of whole blocks goes through the
// whole shard or the whole object instead.
bool sub_shard_ok(const ShardPlacement& s, const gpu::RangePiece& p) {
  switch (s.storage_class) {
    case StorageClass::NVME:
    case StorageClass::SSD:
    case StorageClass::HDD:
      return (s.offset + p.shard_off) % 4096 == 0 &&
             (p.nbytes % 4096 == 0 || p.shard_off + p.nbytes == s.length);
    default:
      return true;
  }
}
}  // namespace

Result<std::string> Client::get_range(const ObjectKey& key, uint64_t offset,
                                      uint64_t length) {
  auto meta = meta_call<KeyMsg, GetWorkersResponse>(M::GET_WORKERS, KeyMsg{key},
                                                     opts_.rpc_timeout_ms);
  if (!meta.ok()) return meta.error();
  if (!range_inside(offset, length, meta->size))
    return Error{ErrorCode::INVALID_ARGUMENT, "range past the end of " + key};
  std::string out;
  out.resize(length);
  Error last{ErrorCode::NO_PLACEMENT, "no copies"};
  for (const auto& copy : meta->copies) {
    auto pieces = gpu::range_pieces(meta->size, shard_lens_of(copy), offset, length);
    if (!pieces) continue;  // the copy does not cover the object
    bool ok = true;
    for (const auto& p : *pieces) {
      const ShardPlacement& s = copy.shards[p.shard];
      char* dst = out.data() + (p.obj_off - offset);
      Result<void> r;
      if (sub_shard_ok(s, p)) {
        r = read_shard(sub_shard(s, p.shard_off, p.nbytes), dst);
      } else {
        std::string whole(s.length, '\0');
        r = read_shard(s, whole.data());
        if (r.ok()) std::memcpy(dst, whole.data() + p.shard_off, p.nbytes);
      }
      if (!r.ok()) {
        ok = false;
        last = r.error();
        break;
      }
    }
    if (ok) return out;
  }
  return last;
}

Result<BatchGetWorkersResponse> Client::patch_start(
    const std::vector<ObjectKey>& keys) {
  auto resp = meta_call<KeysMsg, BatchGetWorkersResponse>(
      M::BATCH_PATCH_START, KeysMsg{keys}, opts_.rpc_timeout_ms);
  if (resp.ok() && resp->items.size() != keys.size())
    return Error{ErrorCode::PROTOCOL_ERROR, "patch start: item count"};
  return resp;
}

void Client::patch_abort(const std::vector<ObjectKey>& keys) {
  if (keys.empty()) return;
  meta_call_raw(M::BATCH_PATCH_ABORT, serde::to_bytes(KeysMsg{keys}),
                opts_.rpc_timeout_ms);
}

Result<void> Client::patch(const ObjectKey& key, uint64_t offset,
                           const void* data, uint64_t size) {
  const uint8_t* new_bytes = static_cast<const uint8_t*>(data);
  // get, overlay, put back: right on every tier and placement
  auto rewrite = [&](const GetWorkersResponse& info) -> Result<void> {
    std::string whole(info.size, '\0');
    BB_RETURN_IF_ERROR(read_copy(info.copies, whole.data(), info.size));
    if (info.checksum != 0 &&
        gpu::checksum_cpu(whole.data(), whole.size()) != info.checksum)
      return Error{ErrorCode::CHECKSUM_MISMATCH, key};
    std::memcpy(whole.data() + offset, new_bytes, size);
    PlacementConfig cfg;
    cfg.replace = true;
    cfg.replication = static_cast<uint32_t>(info.copies.size());
    for (const auto& c : info.copies)
      cfg.max_workers_per_copy = std::max<uint32_t>(
          cfg.max_workers_per_copy, static_cast<uint32_t>(c.shards.size()));
    if (!info.copies.empty() && !info.copies[0].shards.empty())
      cfg.preferred_class = info.copies[0].shards[0].storage_class;
    return put(key, whole.data(), whole.size(), cfg);
  };
  auto in_range = [&](uint64_t obj_size) {
    return range_inside(offset, size, obj_size);
  };

  auto started = patch_start({key});
  if (!started.ok()) return started.error();
  const auto& item = started->items[0];
  if (item.status == static_cast<int32_t>(ErrorCode::INVALID_STATE)) {
    // no recorded checksum: nothing to move, and no state was changed
    auto meta = meta_call<KeyMsg, GetWorkersResponse>(M::GET_WORKERS, KeyMsg{key},
                                                       opts_.rpc_timeout_ms);
    if (!meta.ok()) return meta.error();
    if (!in_range(meta->size))
      return Error{ErrorCode::INVALID_ARGUMENT, "range past the end of " + key};
    return rewrite(meta.value());
  }
  if (item.status != 0)
    return Error{static_cast<ErrorCode>(item.status), key};
  const GetWorkersResponse& info = item.info;
  if (!in_range(info.size)) {
    patch_abort({key});
    return Error{ErrorCode::INVALID_ARGUMENT, "range past the end of " + key};
  }

  using digest::kTileBytes;
  // a piece rounded out to whole tiles of its shard, clipped at the shard's
  // end: what has to be read to move the digests by it. A piece of whole
  // tiles, or one from a tile boundary to the object's end, is its own.
  auto rounded = [](const gpu::RangePiece& p, uint64_t shard_len) {
    const uint64_t head = p.shard_off % kTileBytes;
    const uint64_t end = p.shard_off + p.nbytes;
    const uint64_t stop = std::min(
        shard_len, (end + kTileBytes - 1) / kTileBytes * kTileBytes);
    return gpu::RangePiece{p.shard, p.shard_off - head, p.obj_off - head,
                           stop - (p.shard_off - head)};
  };
  // every copy's pieces, or the rewrite route
  std::vector<std::vector<gpu::RangePiece>> plans;
  bool in_place = !info.copies.empty();
  for (const auto& copy : info.copies) {
    std::optional<std::vector<gpu::RangePiece>> pieces;
    if (opts_.patch_edge_tiles) {
      // runs and edge tiles of one shard lie back to back: the bytes written
      // there are one piece again, in shard order
      if (auto plan = gpu::plan_patch_bytes(info.size, shard_lens_of(copy),
                                            offset, size)) {
        std::vector<gpu::RangePiece> all = std::move(plan->runs);
        for (const auto& e : plan->edges)
          all.push_back({e.shard, e.shard_tile * kTileBytes + e.lo,
                         e.obj_tile * kTileBytes + e.lo, uint64_t{e.hi} - e.lo});
        std::sort(all.begin(), all.end(), [](const auto& a, const auto& b) {
          return a.obj_off < b.obj_off;
        });
        pieces.emplace();
        for (const auto& p : all) {
          if (!pieces->empty() && pieces->back().shard == p.shard)
            pieces->back().nbytes += p.nbytes;
          else
            pieces->push_back(p);
        }
      }
    } else {
      pieces = gpu::plan_patch(info.size, shard_lens_of(copy), offset, size);
    }
    if (!pieces) {
      in_place = false;
      break;
    }
    for (const auto& s : copy.shards)
      if (s.digest == 0) in_place = false;
    for (const auto& p : *pieces) {
      const auto& shard = copy.shards[p.shard];
      if (!sub_shard_ok(shard, p) ||
          !sub_shard_ok(shard, rounded(p, shard.length)))
        in_place = false;
    }
    plans.push_back(std::move(*pieces));
  }
  if (!in_place) {
    patch_abort({key});
    return rewrite(info);
  }

  // old bytes first — nothing is written until every copy's new digests are
  // known and agree
  PutCompleteRequest done_req{key, 0, {}};
  std::string old(size, '\0');
  std::string edge_old, edge_new;  // a piece with edge tiles, rounded out
  for (size_t c = 0; c < info.copies.size(); ++c) {
    const auto& copy = info.copies[c];
    uint64_t h = gpu::checksum_cpu_unfinalize(info.checksum, info.size);
    std::vector<uint64_t> sums;
    for (const auto& s : copy.shards)
      sums.push_back(gpu::checksum_cpu_unfinalize(s.digest, s.length));
    for (const auto& p : plans[c]) {
      const uint64_t at = p.obj_off - offset;
      // the tiles the piece touches: their old bytes, and what they become
      const gpu::RangePiece t = rounded(p, copy.shards[p.shard].length);
      const bool edges = t.nbytes != p.nbytes;
      char* old_t = old.data() + at;
      const void* new_t = new_bytes + at;
      if (edges) {
        edge_old.resize(t.nbytes);
        old_t = edge_old.data();
      }
      auto r = read_shard(sub_shard(copy.shards[p.shard], t.shard_off, t.nbytes),
                          old_t);
      if (!r.ok()) {
        patch_abort({key});
        return r.error();
      }
      if (edges) {  // composed of old and new bytes
        edge_new = edge_old;
        std::memcpy(edge_new.data() + (p.shard_off - t.shard_off),
                    new_bytes + at, p.nbytes);
        new_t = edge_new.data();
      }
      const uint64_t ot = t.obj_off / kTileBytes, st = t.shard_off / kTileBytes;
      h += gpu::checksum_cpu_tiles(new_t, t.nbytes, ot) -
           gpu::checksum_cpu_tiles(old_t, t.nbytes, ot);
      sums[p.shard] += gpu::checksum_cpu_tiles(new_t, t.nbytes, st) -
                       gpu::checksum_cpu_tiles(old_t, t.nbytes, st);
    }
    const uint64_t checksum = gpu::checksum_cpu_finalize(h, info.size);
    if (c > 0 && checksum != done_req.checksum) {
      patch_abort({key});
      return Error{ErrorCode::CHECKSUM_MISMATCH, "replicas of " + key + " diverged"};
    }
    done_req.checksum = checksum;
    for (size_t s = 0; s < sums.size(); ++s)
      sums[s] = gpu::checksum_cpu_finalize(sums[s], copy.shards[s].length);
    done_req.shard_digests.push_back(std::move(sums));
  }
  for (size_t c = 0; c < info.copies.size(); ++c)
    for (const auto& p : plans[c]) {
      auto r = write_shard(
          sub_shard(info.copies[c].shards[p.shard], p.shard_off, p.nbytes),
          new_bytes + (p.obj_off - offset));
      if (!r.ok()) {  // torn
        cancel_puts({key});
        return r.error();
      }
    }
  auto done = meta_call_raw(M::BATCH_PUT_COMPLETE,
                            serde::to_bytes(PutCompleteListMsg{{done_req}}),
                            opts_.rpc_timeout_ms);
  if (!done.ok()) return done.error();
  StatusListMsg st;
  if (!serde::from_bytes(done.value(), st) || st.statuses.size() != 1)
    return Error{ErrorCode::PROTOCOL_ERROR, "patch commit answer"};
  if (st.statuses[0] != 0)
    return Error{static_cast<ErrorCode>(st.statuses[0]), key};
  return {};
}

Result<bool> Client::exists(const ObjectKey& key) {
  auto r = meta_call<KeyMsg, BoolMsg>(M::OBJECT_EXISTS, KeyMsg{key},
                                       opts_.rpc_timeout_ms);
  if (!r.ok()) return r.error();
  return r->v != 0;
}

Result<void> Client::remove(const ObjectKey& key) {
  const uint64_t gen = reconnect_gen_.load();
  auto r = meta_call_raw(M::REMOVE_OBJECT, serde::to_bytes(KeyMsg{key}),
                          opts_.rpc_timeout_ms);
  if (!r.ok()) {
    // see batch_remove: NOT_FOUND after an in-call failover = already gone
    if (r.code() == ErrorCode::OBJECT_NOT_FOUND &&
        reconnect_gen_.load() != gen)
      return {};
    return r.error();
  }
  return {};
}

Result<uint64_t> Client::remove_all() {
  auto r = meta_call_raw(M::REMOVE_ALL_OBJECTS, {}, opts_.rpc_timeout_ms);
  if (!r.ok()) return r.error();
  U64Msg m;
  serde::from_bytes(r.value(), m);
  return m.v;
}

// ------------------------------------------------------------- batch ops

Result<std::vector<int32_t>> Client::batch_remove(
    const std::vector<ObjectKey>& keys) {
  const uint64_t gen = reconnect_gen_.load();
  auto r = meta_call<KeysMsg, StatusListMsg>(M::BATCH_REMOVE, KeysMsg{keys},
                                              opts_.rpc_timeout_ms);
  if (!r.ok()) return r.error();
  if (reconnect_gen_.load() != gen) {
    // a leader failover happened inside this call: the first attempt may
    // have applied + replicated before the reply was lost, so the retried
    // remove sees NOT_FOUND — the intent (key gone) is satisfied
    for (auto& st : r->statuses)
      if (st == static_cast<int32_t>(ErrorCode::OBJECT_NOT_FOUND)) st = 0;
  }
  return std::move(r->statuses);
}



bool Client::failover_retriable(int32_t st) {
  switch (static_cast<ErrorCode>(st)) {
    case ErrorCode::OBJECT_NOT_FOUND:   // new leader never saw the PENDING put
    case ErrorCode::INVALID_STATE:      // replace-put interrupted between
                                        // start and commit: the new leader
                                        // restored the PREVIOUS committed
                                        // digest, so our commit looks like a
                                        // different-content double-commit —
                                        // a full redo re-places + rewrites
    case ErrorCode::NOT_LEADER:
    case ErrorCode::NOT_CONNECTED:
    case ErrorCode::CONNECT_FAILED:
    case ErrorCode::CONNECTION_CLOSED:
    case ErrorCode::SEND_FAILED:
    case ErrorCode::RECV_FAILED:
    case ErrorCode::RPC_FAILED:
      return true;
    default:
      return false;
  }
}

Result<std::vector<int32_t>> Client::batch_put(const std::vector<PutItem>& items,
                                               const PlacementConfig& cfg,
                                               HostPutSession* sess) {
  if (auto fast = try_host_session_put(items, sess)) return std::move(*fast);
  return redo_after_failover(items, [&](const auto& its, bool first) {
    return batch_put_once(its, cfg, first ? sess : nullptr);
  });
}

// ---- put epilogues shared by the host and GPU paths (v1 and v2) ----

Result<void> Client::commit_by_token(uint64_t token, bool release,
                                     const uint64_t* digests, size_t n,
                                     size_t stride) {
  auto r = meta_call_raw(
      M::BATCH_COMMIT_TOKEN,
      wire::encode_commit_token(token, release, digests, n, stride));
  if (!r.ok()) return r.error();
  return {};
}

Result<void> Client::commit_by_token_shards(uint64_t token, bool release,
                                            const uint64_t* obj_digests,
                                            size_t n,
                                            const uint64_t* shard_digests,
                                            size_t m) {
  auto r = meta_call_raw(M::BATCH_COMMIT_TOKEN_SHARDS,
                         wire::encode_commit_token_shards(
                             token, release, obj_digests, n, shard_digests, m));
  if (!r.ok()) return r.error();
  return {};
}

Result<uint64_t> Client::open_session(
    const std::vector<std::pair<ObjectKey, uint64_t>>& objects,
    bool allow_striped) {
  struct Item {
    const ObjectKey& key;
    uint64_t size;
  };
  std::vector<Item> items;
  items.reserve(objects.size());
  for (const auto& [key, size] : objects) items.push_back({key, size});
  auto r = meta_call_raw(M::BATCH_SESSION_OPEN,
                         wire::encode_session_open(items, allow_striped));
  if (!r.ok()) return r.error();
  return wire::decode_session_open_response(r.value());
}

Result<wire::PatchStartDigests> Client::patch_start_token(uint64_t token) {
  auto r = meta_call_raw(M::BATCH_PATCH_START_TOKEN,
                         wire::encode_patch_start_token(token));
  if (!r.ok()) return r.error();
  return wire::decode_patch_start_token_response(r.value());
}

Result<void> Client::complete_by_keys(
    const std::vector<PutCompleteRequest>& reqs,
    const std::vector<uint32_t>& order, std::vector<int32_t>* statuses) {
  if (reqs.empty()) return {};
  // (a bare vector encodes exactly like a one-field list message)
  auto r = meta_call<std::vector<PutCompleteRequest>, StatusListMsg>(
      M::BATCH_PUT_COMPLETE, reqs);
  if (!r.ok()) return r.error();
  // per-item commit failures (e.g. a failover lost the PENDING state) must
  // reach the caller, not vanish
  if (statuses)
    for (size_t j = 0; j < order.size() && j < r->statuses.size(); ++j)
      if (r->statuses[j] != 0) (*statuses)[order[j]] = r->statuses[j];
  return {};
}

void Client::cancel_puts(const std::vector<ObjectKey>& keys) {
  if (!keys.empty())
    meta_call_raw(M::BATCH_PUT_CANCEL, serde::to_bytes(KeysMsg{keys}));
}

// ---- put epilogue of the host paths (v1 and v2) ----

Result<void> Client::finish_puts(
    const std::vector<PutItem>& items, const std::vector<uint64_t>& digests,
    std::vector<int32_t>& statuses,
    const std::function<std::vector<std::vector<uint64_t>>(size_t)>&
        shard_digests_of,
    const std::function<bool(size_t)>& cancellable) {
  std::vector<PutCompleteRequest> completes;
  std::vector<ObjectKey> cancels;
  std::vector<uint32_t> complete_idx;
  for (size_t i = 0; i < items.size(); ++i) {
    if (statuses[i] != 0) {
      if (cancellable(i)) cancels.push_back(items[i].key);
      continue;
    }
    PutCompleteRequest pc{items[i].key, digests[i], {}};
    if (shard_digests_of) pc.shard_digests = shard_digests_of(i);
    completes.push_back(std::move(pc));
    complete_idx.push_back(static_cast<uint32_t>(i));
  }
  BB_RETURN_IF_ERROR(complete_by_keys(completes, complete_idx, &statuses));
  cancel_puts(cancels);
  return {};
}

// Token fast path for the host tier: placements unchanged since the last
// step ⇒ two tiny RPCs around direct memcpys + CPU digests. Mirrors
// GpuClient::try_session_put, including the ordering guarantee: the server
// flips the session's objects to PENDING (pinning the placements) BEFORE
// any byte is written.
std::optional<std::vector<int32_t>> Client::try_host_session_put(
    const std::vector<PutItem>& items, HostPutSession* sess) {
  if (!sess || sess->token == 0 || sess->owner != this || items.empty())
    return std::nullopt;
  const uint32_t dpi = std::max<uint32_t>(sess->dsts_per_item, 1);
  if (sess->srcs.size() != items.size() ||
      sess->dsts.size() != items.size() * dpi)
    return std::nullopt;
  for (size_t i = 0; i < items.size(); ++i)
    if (sess->srcs[i] != items[i].data || sess->sizes[i] != items[i].size) {
      sess->token = 0;
      return std::nullopt;
    }
  auto r1 = meta_call_raw(M::BATCH_UPSERT_START,
                          wire::encode_upsert_start(sess->token));
  if (!r1.ok()) {
    sess->token = 0;  // stale before any write: clean fallback
    return std::nullopt;
  }
  std::vector<uint64_t> digests(items.size(), 0);
  fan_out(items.size(), opts_.io_threads, [&](size_t i) {
    for (uint32_t k = 0; k < dpi; ++k)
      std::memcpy(sess->dsts[i * dpi + k], items[i].data, items[i].size);
    digests[i] = gpu::checksum_cpu(items[i].data, items[i].size);
  });
  auto r2 = commit_by_token(sess->token, /*release=*/false, digests.data(),
                            digests.size());
  if (!r2.ok()) {
    sess->token = 0;  // placements changed mid-step: full path re-places
    return std::nullopt;
  }
  host_session_steps_.fetch_add(1);
  return std::vector<int32_t>(items.size(), 0);
}

uint8_t* Client::host_pool_base(const PoolId& id, AccessInfo* access) {
  PoolView v = PoolMapper::local(id);
  if (!v.base) {
    auto a = pool_access(id);
    if (!a.ok()) return nullptr;
    // device pools stay on the shard path (write_shard/read_shard
    // hipMemcpy), which imports them when it first needs them
    if (a->kind != AccessKind::HIP_IPC) v = mapper_->remote(a.value());
    if (access) *access = std::move(a.value());
  }
  return v.device ? nullptr : v.base;
}

// Host twin of GpuClient::batch_put_device_v2: compact request, pool-table
// response, memcpy into mapped pools (shard RPC fallback), digests computed
// on the fly, commit by one-shot token when the whole batch qualifies —
// BATCH_PUT_COMPLETE never re-sends keys on the common path.
Result<std::vector<int32_t>> Client::batch_put_once_v2(
    const std::vector<PutItem>& items, const PlacementConfig& cfg,
    HostPutSession* sess) {
  const bool establish =
      sess != nullptr && cfg.replace && cfg.checksum && !opts_.force_tcp;
  const bool want_token = establish || cfg.checksum;
  auto resp = meta_call_raw(
      M::BATCH_PUT_START2,
      wire::encode_put_start2_request(items, cfg, want_token));
  if (!resp.ok()) return resp.error();
  wire::BatchPlacements pl;
  BB_RETURN_IF_ERROR(
      wire::decode_put_start2_response(resp.value(), items.size(), pl));
  const uint64_t token = pl.token;
  const auto pools = resolve_pool_table(
      pl.pools,
      [this](const PoolId& id, AccessInfo* a) { return host_pool_base(id, a); });

  std::vector<int32_t> statuses(items.size(), 0);
  for (size_t i = 0; i < items.size(); ++i) {
    statuses[i] = pl.items[i].status;
    // a placement naming a pool outside the table fails the item
    for (uint8_t c = 0; c < pl.items[i].ncopies; ++c)
      if (pl.places_of(pl.items[i])[c].pool_idx >= pools.size())
        statuses[i] = static_cast<int32_t>(ErrorCode::PROTOCOL_ERROR);
  }

  // establishment bookkeeping: one dst per copy per item, all host-mapped
  const uint32_t dpi = std::max<uint32_t>(cfg.replication, 1);
  std::vector<uint8_t*> sess_dsts;
  bool all_mapped = establish;
  if (establish) {
    sess_dsts.assign(items.size() * dpi, nullptr);
    for (size_t i = 0; i < items.size() && all_mapped; ++i) {
      if (statuses[i] != 0 || pl.items[i].ncopies != dpi) {
        all_mapped = false;
        break;
      }
      for (uint32_t k = 0; k < dpi; ++k) {
        const wire::Place& p = pl.places_of(pl.items[i])[k];
        if (!pools[p.pool_idx].base) {
          all_mapped = false;
          break;
        }
        sess_dsts[i * dpi + k] = pools[p.pool_idx].base + p.offset;
      }
    }
  }

  // transfers + digests fan out per item (digest runs while the bytes are
  // still cache-hot from the memcpy)
  std::vector<uint64_t> digests(items.size(), 0);
  fan_out(items.size(), opts_.io_threads, [&](size_t i) {
    if (statuses[i] != 0) return;
    for (uint8_t c = 0; c < pl.items[i].ncopies; ++c) {
      const wire::Place& p = pl.places_of(pl.items[i])[c];
      const PoolRef& pr = pools[p.pool_idx];
      if (pr.base) {
        std::memcpy(pr.base + p.offset, items[i].data, items[i].size);
      } else {
        auto r = write_shard(pr.shard(p.offset, items[i].size), items[i].data);
        if (!r.ok()) {
          statuses[i] = static_cast<int32_t>(r.code());
          break;
        }
      }
    }
    if (cfg.checksum && statuses[i] == 0)
      digests[i] = gpu::checksum_cpu(items[i].data, items[i].size);
  });

  bool all_ok = token != 0;
  for (auto st : statuses)
    if (st != 0) { all_ok = false; break; }
  const bool keep_session = all_ok && establish && all_mapped;
  // one-shot unless establishing
  const bool committed =
      all_ok && commit_by_token(token, /*release=*/!keep_session,
                                digests.data(), digests.size()).ok();
  if (keep_session && committed) {
    sess->token = token;
    sess->dsts_per_item = dpi;
    sess->dsts = std::move(sess_dsts);
    sess->srcs.clear();
    sess->sizes.clear();
    sess->srcs.reserve(items.size());
    sess->sizes.reserve(items.size());
    for (const auto& it : items) {
      sess->srcs.push_back(it.data);
      sess->sizes.push_back(it.size);
    }
    sess->owner = this;
  } else if (sess) {
    sess->token = 0;
  }
  if (!committed) {
    auto cancellable = [&](size_t i) {
      return statuses[i] != static_cast<int32_t>(ErrorCode::OBJECT_EXISTS) &&
             statuses[i] != static_cast<int32_t>(ErrorCode::NO_SPACE);
    };
    BB_RETURN_IF_ERROR(
        finish_puts(items, digests, statuses, nullptr, cancellable));
  }
  return statuses;
}

Result<std::vector<std::pair<int32_t, std::string>>> Client::batch_get_once_v2(
    const std::vector<ObjectKey>& keys, bool* fallback) {
  *fallback = false;
  auto resp = meta_call_raw(M::BATCH_GET_WORKERS2,
                            wire::encode_get_workers2_request(keys));
  if (!resp.ok()) return resp.error();
  wire::BatchPlacements pl;
  BB_RETURN_IF_ERROR(
      wire::decode_get_workers2_response(resp.value(), keys.size(), pl));
  const auto pools = resolve_pool_table(
      pl.pools,
      [this](const PoolId& id, AccessInfo* a) { return host_pool_base(id, a); });

  std::vector<std::pair<int32_t, std::string>> out(keys.size());
  for (size_t i = 0; i < keys.size(); ++i) {
    out[i].first = pl.items[i].status;
    if (out[i].first == static_cast<int32_t>(ErrorCode::NOT_IMPLEMENTED))
      *fallback = true;  // striped object in the batch: run the v1 path
    if (out[i].first == 0) out[i].second.resize(pl.items[i].size);
  }
  if (*fallback) return out;

  fan_out(keys.size(), opts_.io_threads, [&](size_t i) {
    if (out[i].first != 0) return;
    const uint64_t size = out[i].second.size();
    Error last{ErrorCode::NO_PLACEMENT, "no copies"};
    bool done = false;
    const uint64_t want = pl.items[i].checksum;
    for (uint8_t c = 0; c < pl.items[i].ncopies; ++c) {
      const wire::Place& p = pl.places_of(pl.items[i])[c];
      if (p.pool_idx >= pools.size()) continue;  // unknown pool: skip copy
      const PoolRef& pr = pools[p.pool_idx];
      if (pr.base) {
        std::memcpy(out[i].second.data(), pr.base + p.offset, size);
        done = true;
      } else {
        auto r = read_shard(pr.shard(p.offset, size), out[i].second.data());
        if (r.ok()) done = true;
        else last = r.error();
      }
      if (done && opts_.verify_checksum_on_get && want != 0) {
        if (gpu::checksum_cpu(out[i].second.data(), size) != want) {
          done = false;  // corrupt copy: try the next one
          last = Error{ErrorCode::CHECKSUM_MISMATCH, keys[i]};
        }
      }
      if (done) break;
    }
    if (!done) {
      out[i].first = static_cast<int32_t>(last.code);
      out[i].second.clear();
    }
  });
  return out;
}

bool Client::bucket_copy(size_t item, const CopyPlacement& copy,
                         EndpointBuckets& out) {
  uint64_t off = 0;
  for (const auto& sh : copy.shards) {
    auto a = pool_access(sh.pool_id);
    if (!a.ok()) return false;
    out[a.value().endpoint].push_back({item, &sh, off});
    off += sh.length;
  }
  return true;
}

Result<std::vector<int32_t>> Client::batch_put_once(const std::vector<PutItem>& items,
                                               const PlacementConfig& cfg,
                                               HostPutSession* sess) {
  if (!opts_.force_tcp && cfg.max_workers_per_copy <= 1 && !items.empty())
    return batch_put_once_v2(items, cfg, sess);
  BatchPutStartRequest breq;
  breq.requests.reserve(items.size());
  for (const auto& it : items)
    breq.requests.push_back(PutStartRequest{it.key, it.size, cfg});
  auto start = meta_call<BatchPutStartRequest, BatchPutStartResponse>(
      M::BATCH_PUT_START, breq, opts_.rpc_timeout_ms);
  if (!start.ok()) return start.error();

  std::vector<int32_t> statuses(items.size(), 0);
  std::vector<uint64_t> digests(items.size(), 0);
  // epilogue of both transfer strategies below: complete what transferred
  // (striped copies carry per-shard digests), cancel what did not; an item
  // whose placement failed is never cancelled
  auto finish = [&]() -> Result<std::vector<int32_t>> {
    std::function<std::vector<std::vector<uint64_t>>(size_t)> shard_digests;
    if (cfg.checksum)
      shard_digests = [&](size_t i) {
        return host_shard_digests(start->items[i].copies, items[i].data);
      };
    BB_RETURN_IF_ERROR(
        finish_puts(items, digests, statuses, shard_digests,
                    [&](size_t i) { return start->items[i].status == 0; }));
    return statuses;
  };

  if (opts_.force_tcp) {
    // one DATA_BATCH_WRITE per worker endpoint instead of one RPC per shard
    EndpointBuckets buckets;
    bool grouped = true;
    for (size_t i = 0; i < items.size() && grouped; ++i) {
      auto& item = start->items[i];
      if (item.status != 0) {
        statuses[i] = item.status;
        continue;
      }
      for (const auto& copy : item.copies)
        if (!(grouped = bucket_copy(i, copy, buckets))) break;
    }
    if (grouped) {
      for (auto& [ep, shards] : buckets) {
        BatchWriteEnc batch;
        for (const auto& [i, sh, off] : shards) {
          WriteReq w;
          w.pool_id = sh->pool_id;
          w.offset = sh->offset;
          w.src = static_cast<const uint8_t*>(items[i].data) + off;
          w.len = sh->length;
          batch.writes.push_back(w);
        }
        auto* dc = data_client(ep);
        Result<std::string> r =
            dc ? dc->call_raw(M::DATA_BATCH_WRITE, serde::to_bytes(batch),
                              opts_.rpc_timeout_ms)
               : Result<std::string>(Error{ErrorCode::CONNECT_FAILED, ep});
        if (!r.ok())
          for (const auto& es : shards)
            statuses[es.item] = static_cast<int32_t>(r.code());
      }
      if (cfg.checksum)
        for (size_t i = 0; i < items.size(); ++i)
          if (statuses[i] == 0 && start->items[i].status == 0)
            digests[i] = gpu::checksum_cpu(items[i].data, items[i].size);
      return finish();
    }
  }

  // transfers + digests fan out across the IO pool (each object independent)
  fan_out(items.size(), opts_.io_threads, [&](size_t i) {
    auto& item = start->items[i];
    if (item.status != 0) {
      statuses[i] = item.status;
      return;
    }
    auto xfer = write_copies(item.copies, items[i].data, items[i].size);
    if (!xfer.ok()) {
      statuses[i] = static_cast<int32_t>(xfer.code());
      return;
    }
    if (cfg.checksum)
      digests[i] = gpu::checksum_cpu(items[i].data, items[i].size);
  });
  return finish();
}

Result<std::vector<std::pair<int32_t, std::string>>> Client::batch_get(
    const std::vector<ObjectKey>& keys) {
  // failover mid-batch: the new leader may briefly lag the persistence
  // stream — failover-shaped per-item failures are redone once
  return redo_after_failover(
      keys, [&](const auto& ks, bool) { return batch_get_once(ks); });
}

Result<std::vector<std::pair<int32_t, std::string>>> Client::batch_get_once(
    const std::vector<ObjectKey>& keys) {
  if (!opts_.force_tcp && !keys.empty()) {
    bool fb = false;
    auto v2 = batch_get_once_v2(keys, &fb);
    if (v2.ok() && !fb) return v2;
    if (!v2.ok()) return v2;  // whole-call errors surface (failover retries
                              // happen one level up in batch_get)
  }
  auto meta = meta_call<KeysMsg, BatchGetWorkersResponse>(
      M::BATCH_GET_WORKERS, KeysMsg{keys}, opts_.rpc_timeout_ms);
  if (!meta.ok()) return meta.error();
  std::vector<std::pair<int32_t, std::string>> out(keys.size());

  if (opts_.force_tcp) {
    // one DATA_BATCH_READ per worker endpoint, of each item's first copy
    EndpointBuckets buckets;
    bool grouped = true;
    for (size_t i = 0; i < keys.size() && grouped; ++i) {
      auto& item = meta->items[i];
      if (item.status != 0) {
        out[i].first = item.status;
        continue;
      }
      out[i].second.resize(item.info.size);
      if (item.info.copies.empty()) {
        out[i].first = static_cast<int32_t>(ErrorCode::NO_PLACEMENT);
        continue;
      }
      grouped = bucket_copy(i, item.info.copies[0], buckets);
    }
    if (grouped) {
      for (const auto& bucket : buckets) {
        const std::string& ep = bucket.first;
        const std::vector<EndpointShard>& shards = bucket.second;
        auto fail = [&](ErrorCode code) {
          for (const auto& es : shards)
            out[es.item].first = static_cast<int32_t>(code);
        };
        BatchReadEnc batch;
        for (const auto& es : shards)
          batch.reads.push_back(
              ReadReq{es.shard->pool_id, es.shard->offset, es.shard->length});
        auto* dc = data_client(ep);
        Result<std::string> r =
            dc ? dc->call_raw(M::DATA_BATCH_READ, serde::to_bytes(batch),
                              opts_.rpc_timeout_ms)
               : Result<std::string>(Error{ErrorCode::CONNECT_FAILED, ep});
        if (!r.ok()) {
          fail(r.code());
          continue;
        }
        serde::Dec d(r.value().data(), r.value().size());
        uint32_t n = d.num<uint32_t>();
        if (n != shards.size()) {
          fail(ErrorCode::PROTOCOL_ERROR);
          continue;
        }
        for (const auto& [i, sh, off] : shards) {
          auto payload = d.bytes();
          if (!d.ok() || payload.size() != sh->length) {
            out[i].first = static_cast<int32_t>(ErrorCode::PROTOCOL_ERROR);
            continue;
          }
          std::memcpy(out[i].second.data() + off, payload.data(), payload.size());
        }
      }
      for (size_t i = 0; i < keys.size(); ++i)
        if (out[i].first != 0) out[i].second.clear();
      return out;
    }
  }

  fan_out(keys.size(), opts_.io_threads, [&](size_t i) {
    auto& item = meta->items[i];
    if (item.status != 0) {
      out[i].first = item.status;
      return;
    }
    out[i].second.resize(item.info.size);
    auto r = read_copy(item.info.copies, out[i].second.data(), item.info.size);
    out[i].first = static_cast<int32_t>(r.code());
    if (!r.ok()) out[i].second.clear();
  });
  return out;
}

// ------------------------------------------------------------ cluster view

Result<ClusterStats> Client::cluster_stats() {
  auto r = meta_call_raw(M::GET_CLUSTER_STATS, {}, opts_.rpc_timeout_ms);
  if (!r.ok()) return r.error();
  ClusterStats s;
  if (!serde::from_bytes(r.value(), s))
    return Error{ErrorCode::PROTOCOL_ERROR, "bad stats"};
  return s;
}

Result<std::vector<MemoryPool>> Client::memory_pools() {
  auto r = meta_call_raw(M::GET_MEMORY_POOLS, {}, opts_.rpc_timeout_ms);
  if (!r.ok()) return r.error();
  PoolsMsg m;
  if (!serde::from_bytes(r.value(), m))
    return Error{ErrorCode::PROTOCOL_ERROR, "bad pools"};
  return std::move(m.pools);
}

Result<std::vector<WorkerInfo>> Client::workers_info() {
  auto r = meta_call_raw(M::GET_WORKERS_INFO, {}, opts_.rpc_timeout_ms);
  if (!r.ok()) return r.error();
  WorkersInfoMsg m;
  if (!serde::from_bytes(r.value(), m))
    return Error{ErrorCode::PROTOCOL_ERROR, "bad workers"};
  return std::move(m.workers);
}

Result<std::vector<ObjectSummary>> Client::list_objects(
    const std::string& prefix, uint32_t limit) {
  serde::Enc e;
  e.str(prefix);
  e.num<uint32_t>(limit);
  auto r = meta_call_raw(M::LIST_OBJECTS, e.buf, opts_.rpc_timeout_ms);
  if (!r.ok()) return r.error();
  serde::Dec d(r.value().data(), r.value().size());
  std::vector<ObjectSummary> out;
  serde::get(d, out);
  if (!d.ok()) return Error{ErrorCode::PROTOCOL_ERROR, "bad list"};
  return out;
}

Result<PingResponse> Client::ping() {
  auto r = meta_call_raw(M::PING, {}, opts_.rpc_timeout_ms);
  if (!r.ok()) return r.error();
  PingResponse p;
  if (!serde::from_bytes(r.value(), p))
    return Error{ErrorCode::PROTOCOL_ERROR, "bad ping"};
  return p;
}

}  // namespace blackbird
