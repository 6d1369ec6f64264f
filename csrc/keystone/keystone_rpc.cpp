#include "blackbird/keystone/keystone_rpc.h"

#include "blackbird/client/batch_wire.h"
#include "blackbird/common/log.h"
#include "blackbird/rpc/messages.h"
#include "blackbird/rpc/methods.h"
#include "blackbird/rpc/net.h"
#include "keystone_internal.h"

namespace blackbird {

namespace {
struct ExistsListMsg {  // BATCH_OBJECT_EXISTS has no caller in this tree yet
  std::vector<uint8_t> exists;
  BB_FIELDS(exists)
};

template <typename Req>
Result<Req> decode(const std::string& body) {
  Req r{};
  if (!serde::from_bytes(body, r))
    return Error{ErrorCode::PROTOCOL_ERROR, "bad request body"};
  return r;
}
}  // namespace

KeystoneServer::KeystoneServer(std::shared_ptr<KeystoneService> service)
    : service_(std::move(service)) {
  register_handlers();
}

KeystoneServer::~KeystoneServer() { stop(); }

void KeystoneServer::register_handlers() {
  namespace M = rpc::methods;
  using Ctx = rpc::RpcServer::ConnCtx;
  using Reply = Result<std::string>;
  auto& ks = *service_;

  // Served by any keystone.
  auto on = [this](uint16_t method, rpc::RpcServer::Handler h) {
    rpc_.register_handler(method, std::move(h));
  };
  // Served by the leader alone. A standby answers with a CALL-level error
  // (for batches too, not per-item statuses), so the client's failover
  // machinery rediscovers the leader and retries.
  auto leader_only = [this, &ks](uint16_t method, auto handler) {
    rpc_.register_handler(
        method, [&ks, handler](const std::string& b, const Ctx& c) -> Reply {
          if (!ks.is_leader()) return not_leader();
          return handler(b, c);
        });
  };

  on(M::PING, [&ks](const std::string&, const Ctx&) -> Reply {
    PingResponse p;
    p.view_version = ks.get_view_version();
    p.server_time_ms = wall_ms();
    p.is_leader = ks.is_leader();
    return serde::to_bytes(p);
  });
  leader_only(M::OBJECT_EXISTS, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<KeyMsg>(b);
    if (!r.ok()) return r.error();
    return serde::to_bytes(BoolMsg{static_cast<uint8_t>(ks.object_exists(r->key))});
  });
  leader_only(M::GET_WORKERS, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<KeyMsg>(b);
    if (!r.ok()) return r.error();
    auto resp = ks.get_workers(r->key);
    if (!resp.ok()) return resp.error();
    return serde::to_bytes(resp.value());
  });
  leader_only(M::PUT_START, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<PutStartRequest>(b);
    if (!r.ok()) return r.error();
    auto resp = ks.put_start(r->key, r->size, r->config);
    if (!resp.ok()) return resp.error();
    return serde::to_bytes(resp.value());
  });
  leader_only(M::PUT_COMPLETE, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<PutCompleteRequest>(b);
    if (!r.ok()) return r.error();
    BB_RETURN_IF_ERROR(ks.put_complete(r->key, r->checksum, r->shard_digests));
    return std::string{};
  });
  leader_only(M::PUT_CANCEL, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<KeyMsg>(b);
    if (!r.ok()) return r.error();
    BB_RETURN_IF_ERROR(ks.put_cancel(r->key));
    return std::string{};
  });
  leader_only(M::REMOVE_OBJECT, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<KeyMsg>(b);
    if (!r.ok()) return r.error();
    BB_RETURN_IF_ERROR(ks.remove_object(r->key));
    return std::string{};
  });
  leader_only(M::REMOVE_ALL_OBJECTS, [&ks](const std::string&, const Ctx&) -> Reply {
    return serde::to_bytes(U64Msg{ks.remove_all_objects()});
  });
  on(M::GET_WORKERS_INFO, [&ks](const std::string&, const Ctx&) -> Reply {
    return serde::to_bytes(WorkersInfoMsg{ks.get_workers_info()});
  });
  on(M::GET_MEMORY_POOLS, [&ks](const std::string&, const Ctx&) -> Reply {
    return serde::to_bytes(PoolsMsg{ks.get_memory_pools()});
  });
  on(M::REMOVE_WORKER, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<KeyMsg>(b);
    if (!r.ok()) return r.error();
    BB_RETURN_IF_ERROR(ks.remove_worker(r->key));
    return std::string{};
  });
  on(M::GET_CLUSTER_STATS, [&ks](const std::string&, const Ctx&) -> Reply {
    return serde::to_bytes(ks.get_cluster_stats());
  });
  on(M::GET_VIEW_VERSION, [&ks](const std::string&, const Ctx&) -> Reply {
    return serde::to_bytes(U64Msg{ks.get_view_version()});
  });
  leader_only(M::LIST_OBJECTS, [&ks](const std::string& b, const Ctx&) -> Reply {
    serde::Dec d(b.data(), b.size());
    std::string prefix = d.str();
    uint32_t limit = d.num<uint32_t>();
    if (!d.ok()) return Error{ErrorCode::PROTOCOL_ERROR, "bad list request"};
    serde::Enc e;
    serde::put(e, ks.list_objects(prefix, limit ? limit : 1000));
    return std::move(e.buf);
  });
  on(M::ADMIN_SCRUB, [&ks](const std::string& b, const Ctx&) -> Reply {
    serde::Dec d(b.data(), b.size());
    uint32_t max_objects = d.num<uint32_t>();
    return serde::to_bytes(U64Msg{ks.run_scrub_once(d.ok() ? max_objects : 0)});
  });
  on(M::ADMIN_REPAIR, [&ks](const std::string&, const Ctx&) -> Reply {
    ks.run_repair_once();
    return std::string{};
  });
  on(M::ADMIN_COMPACT, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<KeyMsg>(b);  // key = pool id
    if (!r.ok()) return r.error();
    auto moved = ks.compact_pool(r->key);
    if (!moved.ok()) return moved.error();
    return serde::to_bytes(U64Msg{moved.value()});
  });
  leader_only(M::BATCH_PUT_START, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<BatchPutStartRequest>(b);
    if (!r.ok()) return r.error();
    return serde::to_bytes(ks.batch_put_start(r->requests));
  });
  leader_only(M::BATCH_PUT_COMPLETE, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<PutCompleteListMsg>(b);
    if (!r.ok()) return r.error();
    return serde::to_bytes(StatusListMsg{ks.batch_put_complete(r->reqs)});
  });
  leader_only(M::BATCH_PUT_CANCEL, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<KeysMsg>(b);
    if (!r.ok()) return r.error();
    return serde::to_bytes(StatusListMsg{ks.batch_put_cancel(r->keys)});
  });
  leader_only(M::BATCH_GET_WORKERS, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<KeysMsg>(b);
    if (!r.ok()) return r.error();
    return serde::to_bytes(ks.batch_get_workers(r->keys));
  });
  leader_only(M::BATCH_PATCH_START, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<KeysMsg>(b);
    if (!r.ok()) return r.error();
    return serde::to_bytes(ks.batch_patch_start(r->keys));
  });
  leader_only(M::BATCH_PATCH_ABORT, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<KeysMsg>(b);
    if (!r.ok()) return r.error();
    return serde::to_bytes(StatusListMsg{ks.batch_patch_abort(r->keys)});
  });
  // ---- compact v2 batch protocol: pool-table + fixed-width placements ----
  leader_only(M::BATCH_PUT_START2, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto rq = wire::decode_put_start2_request(b);
    if (!rq.ok()) return rq.error();
    rq->cfg.max_workers_per_copy = 1;  // v2 contract: single-shard copies
    std::vector<PutStartRequest> reqs;
    reqs.reserve(rq->keys.size());
    for (size_t i = 0; i < rq->keys.size(); ++i)
      reqs.push_back({std::move(rq->keys[i]), rq->sizes[i], rq->cfg});
    auto resp = ks.batch_put_start(reqs);

    wire::BatchPlacements out;
    out.view_version = resp.view_version;
    if (rq->want_token) {
      bool all_ok = !resp.items.empty();
      for (auto& it : resp.items)
        if (it.status != 0) { all_ok = false; break; }
      if (all_ok) out.token = ks.create_put_session(reqs);
    }
    wire::PoolTable table(out.pools);
    for (auto& it : resp.items)
      wire::append_item(out, table, it.status, it.copies);
    return wire::encode_put_start2_response(out);
  });
  leader_only(M::BATCH_GET_WORKERS2, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto keys = wire::decode_get_workers2_request(b);
    if (!keys.ok()) return keys.error();
    auto resp = ks.batch_get_workers(keys.value());

    wire::BatchPlacements out;
    wire::PoolTable table(out.pools);
    for (auto& it : resp.items) {
      // multi-shard copies cannot be encoded in v2 — signal fallback
      int32_t status = it.status;
      for (auto& c : it.info.copies)
        if (status == 0 && c.shards.size() != 1)
          status = static_cast<int32_t>(ErrorCode::NOT_IMPLEMENTED);
      wire::append_item(out, table, status, it.info.copies, it.info.size,
                        it.info.checksum);
    }
    return wire::encode_get_workers2_response(out);
  });
  // the session calls refuse a standby themselves
  on(M::BATCH_UPSERT_START, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto token = wire::decode_upsert_start(b);
    if (!token.ok()) return token.error();
    BB_RETURN_IF_ERROR(ks.upsert_start_token(token.value()));
    return std::string{};
  });
  on(M::BATCH_COMMIT_TOKEN, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto c = wire::decode_commit_token(b);
    if (!c.ok()) return c.error();
    BB_RETURN_IF_ERROR(ks.commit_token(c->token, c->digests, c->flags & 1));
    return std::string{};
  });
  on(M::BATCH_SESSION_OPEN, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto rq = wire::decode_session_open(b);
    if (!rq.ok()) return rq.error();
    std::vector<PutStartRequest> reqs;
    reqs.reserve(rq->keys.size());
    for (size_t i = 0; i < rq->keys.size(); ++i)
      reqs.push_back({std::move(rq->keys[i]), rq->sizes[i], {}});
    auto token = ks.open_session(reqs, rq->flags & 1);
    if (!token.ok()) return token.error();
    return wire::encode_session_open_response(token.value());
  });
  on(M::BATCH_COMMIT_TOKEN_SHARDS, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto c = wire::decode_commit_token_shards(b);
    if (!c.ok()) return c.error();
    BB_RETURN_IF_ERROR(ks.commit_token_shards(c->token, c->obj_digests,
                                              c->shard_digests, c->flags & 1));
    return std::string{};
  });
  on(M::BATCH_PATCH_START_TOKEN, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto token = wire::decode_patch_start_token(b);
    if (!token.ok()) return token.error();
    auto old = ks.patch_start_token(token.value());
    if (!old.ok()) return old.error();
    return wire::encode_patch_start_token_response(
        {std::move(old->obj_digests), std::move(old->shard_digests)});
  });
  leader_only(M::BATCH_REMOVE,[&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<KeysMsg>(b);
    if (!r.ok()) return r.error();
    return serde::to_bytes(StatusListMsg{ks.batch_remove(r->keys)});
  });
  leader_only(M::BATCH_OBJECT_EXISTS, [&ks](const std::string& b, const Ctx&) -> Reply {
    auto r = decode<KeysMsg>(b);
    if (!r.ok()) return r.error();
    return serde::to_bytes(ExistsListMsg{ks.batch_object_exists(r->keys)});
  });
}

Result<void> KeystoneServer::start() {
  const auto& addr = service_->config().listen_address;
  if (net::is_unix_endpoint(addr)) {
    BB_RETURN_IF_ERROR(rpc_.start(addr, 0));
    service_->set_advertised_endpoint(addr);
    BB_LOG(INFO) << "keystone RPC listening on " << addr;
  } else {
    auto hp = net::split_endpoint(addr);
    if (!hp.ok()) return hp.error();
    BB_RETURN_IF_ERROR(rpc_.start(hp.value().first, hp.value().second));
    service_->set_advertised_endpoint(rpc_.endpoint());
    BB_LOG(INFO) << "keystone RPC listening on " << rpc_.endpoint();
  }
  if (!service_->config().metrics_address.empty()) {
    metrics_ = std::make_unique<MetricsHttpServer>(*service_);
    auto mr = metrics_->start(service_->config().metrics_address);
    if (!mr.ok())
      BB_LOG(WARN) << "metrics server failed to start: " << mr.message();
  }
  return {};
}

void KeystoneServer::stop() {
  if (metrics_) metrics_->stop();
  rpc_.stop();
}

Result<std::shared_ptr<KeystoneServer>> create_and_start_keystone(
    const KeystoneConfig& config, std::shared_ptr<coord::CoordService> coord) {
  auto svc = std::make_shared<KeystoneService>(config, std::move(coord));
  BB_RETURN_IF_ERROR(svc->initialize());
  BB_RETURN_IF_ERROR(svc->start());
  auto server = std::make_shared<KeystoneServer>(svc);
  auto r = server->start();
  if (!r.ok()) {
    svc->stop();
    return r.error();
  }
  return server;
}

}  // namespace blackbird
