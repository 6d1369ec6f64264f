// pybind11 bindings: the Python surface of the MI355X-native object store.
// Python is the test/benchmark harness; all logic lives in the C++/HIP core.
#include <pybind11/functional.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "blackbird/allocation/pool_allocator.h"
#include "blackbird/allocation/range_allocator.h"
#include "blackbird/client/batch_wire.h"
#include "blackbird/common/result.h"
#include "blackbird/common/types.h"
#include "blackbird/coord/coord.h"
#include "blackbird/gpu/gpu_kernels.h"

namespace py = pybind11;
using namespace blackbird;

namespace {

class BlackbirdError : public std::runtime_error {
 public:
  BlackbirdError(ErrorCode code, const std::string& msg)
      : std::runtime_error(std::string(to_string(code)) +
                           (msg.empty() ? "" : (": " + msg))),
        code_(code) {}
  ErrorCode code_;
};

template <typename T>
T unwrap(Result<T>&& r) {
  if (!r.ok()) throw BlackbirdError(r.code(), r.message());
  return std::move(r.value());
}

inline void unwrap_void(Result<void>&& r) {
  if (!r.ok()) throw BlackbirdError(r.code(), r.message());
}

}  // namespace

void bind_store(py::module_& m);  // keystone/worker/client (py_store.cpp)

PYBIND11_MODULE(_core, m) {
  m.doc() = "blackbird_amd core — MI355X-native tiered distributed object store";

  static py::exception<BlackbirdError> exc(m, "BlackbirdError");
  py::register_exception_translator([](std::exception_ptr p) {
    try {
      if (p) std::rethrow_exception(p);
    } catch (const BlackbirdError& e) {
      py::set_error(exc, e.what());
    }
  });

  // ------------------------------------------------------------ enums
  py::enum_<StorageClass>(m, "StorageClass")
      .value("RAM_CPU", StorageClass::RAM_CPU)
      .value("RAM_GPU", StorageClass::RAM_GPU)
      .value("PINNED_CPU", StorageClass::PINNED_CPU)
      .value("NVME", StorageClass::NVME)
      .value("SSD", StorageClass::SSD)
      .value("HDD", StorageClass::HDD)
      .value("CXL_MEM", StorageClass::CXL_MEM);

  py::enum_<AccessKind>(m, "AccessKind")
      .value("TCP", AccessKind::TCP)
      .value("SHM", AccessKind::SHM)
      .value("HIP_IPC", AccessKind::HIP_IPC);

  // ------------------------------------------------------------ structs
  py::class_<AccessInfo>(m, "AccessInfo")
      .def(py::init<>())
      .def_readwrite("kind", &AccessInfo::kind)
      .def_readwrite("endpoint", &AccessInfo::endpoint)
      .def_readwrite("shm_name", &AccessInfo::shm_name)
      .def_readwrite("device_id", &AccessInfo::device_id)
      .def_readwrite("ipc_handle_hex", &AccessInfo::ipc_handle_hex)
      .def_readwrite("base_addr", &AccessInfo::base_addr);

  py::class_<MemoryPool>(m, "MemoryPool")
      .def(py::init<>())
      .def_readwrite("pool_id", &MemoryPool::pool_id)
      .def_readwrite("worker_id", &MemoryPool::worker_id)
      .def_readwrite("node_id", &MemoryPool::node_id)
      .def_readwrite("storage_class", &MemoryPool::storage_class)
      .def_readwrite("size", &MemoryPool::size)
      .def_readwrite("used", &MemoryPool::used)
      .def_readwrite("access", &MemoryPool::access)
      .def("to_json", [](const MemoryPool& p) { return p.to_json().dump(); })
      .def_static("from_json", [](const std::string& s) {
        return MemoryPool::from_json(json::parse_or_null(s));
      });

  py::class_<ShardPlacement>(m, "ShardPlacement")
      .def(py::init<>())
      .def_readwrite("pool_id", &ShardPlacement::pool_id)
      .def_readwrite("worker_id", &ShardPlacement::worker_id)
      .def_readwrite("storage_class", &ShardPlacement::storage_class)
      .def_readwrite("offset", &ShardPlacement::offset)
      .def_readwrite("length", &ShardPlacement::length)
      .def_readwrite("access", &ShardPlacement::access)
      .def_readwrite("digest", &ShardPlacement::digest);

  py::class_<CopyPlacement>(m, "CopyPlacement")
      .def(py::init<>())
      .def_readwrite("copy_index", &CopyPlacement::copy_index)
      .def_readwrite("shards", &CopyPlacement::shards);

  py::class_<PlacementConfig>(m, "PlacementConfig")
      .def(py::init<>())
      .def_readwrite("replication", &PlacementConfig::replication)
      .def_readwrite("max_workers_per_copy", &PlacementConfig::max_workers_per_copy)
      .def_readwrite("min_shard_size", &PlacementConfig::min_shard_size)
      .def_readwrite("preferred_class", &PlacementConfig::preferred_class)
      .def_readwrite("required_class", &PlacementConfig::required_class)
      .def_readwrite("ttl_ms", &PlacementConfig::ttl_ms)
      .def_readwrite("checksum", &PlacementConfig::checksum)
      .def_readwrite("preferred_worker", &PlacementConfig::preferred_worker)
      .def_readwrite("replace", &PlacementConfig::replace);

  py::class_<PoolAllocatorStats>(m, "PoolAllocatorStats")
      .def_readonly("capacity", &PoolAllocatorStats::capacity)
      .def_readonly("used", &PoolAllocatorStats::used)
      .def_readonly("free_ranges", &PoolAllocatorStats::free_ranges)
      .def_readonly("largest_free", &PoolAllocatorStats::largest_free)
      .def_readonly("fragmentation", &PoolAllocatorStats::fragmentation);

  py::class_<AllocatorStats>(m, "AllocatorStats")
      .def_readonly("total_capacity", &AllocatorStats::total_capacity)
      .def_readonly("total_used", &AllocatorStats::total_used)
      .def_readonly("num_pools", &AllocatorStats::num_pools)
      .def_readonly("num_objects", &AllocatorStats::num_objects)
      .def_readonly("fragmentation", &AllocatorStats::fragmentation);

  // --------------------------------------------------------- allocators
  py::class_<PoolAllocator>(m, "PoolAllocator")
      .def(py::init([](uint64_t cap, const std::string& policy, uint64_t align) {
             return std::make_unique<PoolAllocator>(
                 cap,
                 policy == "first_fit" ? PoolAllocator::Policy::FIRST_FIT
                                       : PoolAllocator::Policy::BEST_FIT,
                 align);
           }),
           py::arg("capacity"), py::arg("policy") = "best_fit",
           py::arg("alignment") = 256)
      .def("allocate", [](PoolAllocator& a, uint64_t size) {
        return unwrap(a.allocate(size));
      })
      .def("free", [](PoolAllocator& a, uint64_t off, uint64_t size) {
        unwrap_void(a.free(off, size));
      })
      .def("reserve_exact", [](PoolAllocator& a, uint64_t off, uint64_t size) {
        unwrap_void(a.reserve_exact(off, size));
      })
      .def("used", &PoolAllocator::used)
      .def("available", &PoolAllocator::available)
      .def_property_readonly("capacity", &PoolAllocator::capacity)
      .def("stats", &PoolAllocator::stats);

  py::class_<RangeAllocator>(m, "RangeAllocator")
      .def(py::init<>())
      .def("upsert_pool", &RangeAllocator::upsert_pool)
      .def("remove_pool", &RangeAllocator::remove_pool)
      .def("pools", &RangeAllocator::pools)
      .def("allocate", [](RangeAllocator& a, const std::string& key, uint64_t size,
                          const PlacementConfig& cfg) {
        return unwrap(a.allocate(key, size, cfg));
      })
      .def("free", [](RangeAllocator& a, const std::string& key) {
        unwrap_void(a.free(key));
      })
      .def("can_allocate", &RangeAllocator::can_allocate)
      .def("allocate_batch", [](RangeAllocator& a,
                                const std::vector<std::string>& keys,
                                const std::vector<uint64_t>& sizes,
                                const PlacementConfig& cfg) {
        auto out = a.allocate_batch(keys, sizes, cfg);
        py::list res;
        for (auto& [st, copies] : out)
          res.append(py::make_tuple(st, copies));
        return res;
      })
      .def("allocate_batch_bench", [](RangeAllocator& a,
                                      const std::vector<std::string>& keys,
                                      uint64_t size, const PlacementConfig& cfg) {
        std::vector<uint64_t> sizes(keys.size(), size);
        py::gil_scoped_release rel;
        auto out = a.allocate_batch(keys, sizes, cfg);
        int ok = 0;
        for (auto& [st, c] : out)
          if (st == 0) ++ok;
        return ok;
      })
      .def("free_keys_bench", [](RangeAllocator& a,
                                 const std::vector<std::string>& keys) {
        py::gil_scoped_release rel;
        for (auto& k : keys) a.free(k);
      })
      .def("stats", &RangeAllocator::stats);

  // --------------------------------------------------------- coordination
  py::enum_<coord::EventType>(m, "EventType")
      .value("PUT", coord::EventType::PUT)
      .value("DELETE", coord::EventType::DELETE)
      .value("EXPIRE", coord::EventType::EXPIRE);

  py::class_<coord::WatchEvent>(m, "WatchEvent")
      .def_readonly("type", &coord::WatchEvent::type)
      .def_readonly("key", &coord::WatchEvent::key)
      .def_readonly("value", &coord::WatchEvent::value);

  py::class_<coord::CoordStore, std::shared_ptr<coord::CoordStore>>(m, "CoordStore")
      .def(py::init<>())
      .def("sweep_now", &coord::CoordStore::sweep_now)
      .def("size", &coord::CoordStore::size)
      .def("put", [](coord::CoordStore& s, const std::string& k,
                     const std::string& v, uint64_t ttl_ms) {
        unwrap_void(s.put(k, v, ttl_ms));
      }, py::arg("key"), py::arg("value"), py::arg("ttl_ms") = 0)
      .def("get", [](coord::CoordStore& s, const std::string& k) {
        return unwrap(s.get(k));
      })
      .def("save", [](coord::CoordStore& s, const std::string& path) {
        unwrap_void(s.save(path));
      })
      .def("load", [](coord::CoordStore& s, const std::string& path) {
        unwrap_void(s.load(path));
      })
      .def("get_prefix",
           [](coord::CoordStore& s, const std::string& p) {
             auto r = s.get_prefix(p);
             if (!r.ok()) throw std::runtime_error(r.error().message);
             std::vector<std::pair<std::string, py::bytes>> out;
             for (auto& kv : r.value())
               out.emplace_back(kv.key, py::bytes(kv.value));
             return out;
           })
      .def("dirty", &coord::CoordStore::dirty)
      .def("epoch", &coord::CoordStore::epoch)
      .def("bump_epoch", &coord::CoordStore::bump_epoch);

  py::class_<coord::CoordService, std::shared_ptr<coord::CoordService>>(m, "CoordService")
      .def("put", [](coord::CoordService& c, const std::string& k,
                     const std::string& v, uint64_t ttl) {
        unwrap_void(c.put(k, v, ttl));
      }, py::arg("key"), py::arg("value"), py::arg("ttl_ms") = 0,
         py::call_guard<py::gil_scoped_release>())
      .def("get", [](coord::CoordService& c, const std::string& k) {
        return unwrap(c.get(k));
      }, py::call_guard<py::gil_scoped_release>())
      .def("delete_", [](coord::CoordService& c, const std::string& k) {
        unwrap_void(c.del(k));
      }, py::call_guard<py::gil_scoped_release>())
      .def("get_prefix", [](coord::CoordService& c, const std::string& p) {
        auto kvs = unwrap(c.get_prefix(p));
        std::vector<std::pair<std::string, std::string>> out;
        for (auto& kv : kvs) out.emplace_back(kv.key, kv.value);
        return out;
      }, py::call_guard<py::gil_scoped_release>())
      .def("cas", [](coord::CoordService& c, const std::string& k,
                     const std::string& expected, bool expect_absent,
                     const std::string& v, uint64_t ttl) {
        return unwrap(c.cas(k, expected, expect_absent, v, ttl));
      }, py::arg("key"), py::arg("expected"), py::arg("expect_absent"),
         py::arg("value"), py::arg("ttl_ms") = 0,
         py::call_guard<py::gil_scoped_release>())
      .def("keep_alive", [](coord::CoordService& c, const std::string& k, uint64_t ttl) {
        unwrap_void(c.keep_alive(k, ttl));
      }, py::call_guard<py::gil_scoped_release>())
      .def("watch_prefix", [](coord::CoordService& c, const std::string& p,
                              py::function cb) {
        // callback invoked from C++ threads → GIL discipline: hold the
        // py::function behind a shared_ptr (C++-side copies must not touch
        // refcounts) and delete it under the GIL.
        std::shared_ptr<py::function> fptr(
            new py::function(std::move(cb)), [](py::function* f) {
              py::gil_scoped_acquire g;
              delete f;
            });
        auto wrapped = [fptr](const coord::WatchEvent& ev) {
          py::gil_scoped_acquire g;
          try {
            (*fptr)(ev);
          } catch (py::error_already_set& e) {
            e.discard_as_unraisable("watch callback");
          }
        };
        return unwrap(c.watch_prefix(p, wrapped));
      })  // keeps GIL: only registers; RPC inside is fast
      .def("unwatch", [](coord::CoordService& c, uint64_t id) {
        unwrap_void(c.unwatch(id));
      }, py::call_guard<py::gil_scoped_release>());

  py::class_<coord::InProcCoord, coord::CoordService,
             std::shared_ptr<coord::InProcCoord>>(m, "InProcCoord")
      .def(py::init([] {
        return std::make_shared<coord::InProcCoord>(
            std::make_shared<coord::CoordStore>());
      }))
      .def(py::init([](std::shared_ptr<coord::CoordStore> store) {
        return std::make_shared<coord::InProcCoord>(std::move(store));
      }))
      .def("store", &coord::InProcCoord::store);

  py::class_<coord::CoordServer>(m, "CoordServer")
      .def(py::init([](std::shared_ptr<coord::CoordStore> store) {
             return std::make_unique<coord::CoordServer>(std::move(store));
           }))
      .def(py::init([] {
        return std::make_unique<coord::CoordServer>(
            std::make_shared<coord::CoordStore>());
      }))
      .def("start", [](coord::CoordServer& s, const std::string& host, uint16_t port) {
        unwrap_void(s.start(host, port));
      }, py::arg("host") = "127.0.0.1", py::arg("port") = 0)
      .def("stop", &coord::CoordServer::stop, py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("port", &coord::CoordServer::port)
      .def_property_readonly("endpoint", &coord::CoordServer::endpoint)
      .def("store", &coord::CoordServer::store)
      .def("set_read_only", &coord::CoordServer::set_read_only)
      .def("read_only", &coord::CoordServer::read_only);

  py::class_<coord::CoordFollower>(m, "CoordFollower")
      .def(py::init([](coord::CoordServer& server,
                       const std::string& primary, uint64_t failover_ms) {
             return std::make_unique<coord::CoordFollower>(
                 server.store(), &server, primary, failover_ms);
           }),
           py::arg("server"), py::arg("primary"),
           py::arg("failover_ms") = 2000, py::keep_alive<1, 2>())
      .def("start", [](coord::CoordFollower& f) { unwrap_void(f.start()); },
           py::call_guard<py::gil_scoped_release>())
      .def("stop", &coord::CoordFollower::stop,
           py::call_guard<py::gil_scoped_release>())
      .def("promoted", &coord::CoordFollower::promoted);

  py::class_<coord::CoordClient, coord::CoordService,
             std::shared_ptr<coord::CoordClient>>(m, "CoordClient")
      .def(py::init<>())
      .def("connect", [](coord::CoordClient& c, const std::string& ep) {
        unwrap_void(c.connect(ep));
      }, py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("observed_epoch",
                             &coord::CoordClient::observed_epoch)
      .def("put_many",
           [](coord::CoordClient& c,
              const std::vector<std::pair<std::string, std::string>>& puts,
              const std::vector<std::string>& dels) {
             std::vector<coord::KV> kvs;
             kvs.reserve(puts.size());
             for (auto& [k, v] : puts) kvs.push_back({k, v});
             py::gil_scoped_release rel;
             unwrap_void(c.put_many(kvs, dels));
           },
           py::arg("puts"), py::arg("dels") = std::vector<std::string>{})
      .def("close", &coord::CoordClient::close,
           py::call_guard<py::gil_scoped_release>());

  py::class_<coord::LeaderElector>(m, "LeaderElector")
      .def(py::init<std::shared_ptr<coord::CoordService>, std::string,
                    std::string, uint64_t>(),
           py::arg("coord"), py::arg("key"), py::arg("candidate_id"),
           py::arg("lease_ms") = 5000)
      .def("start", &coord::LeaderElector::start)
      .def("stop", &coord::LeaderElector::stop,
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("is_leader", &coord::LeaderElector::is_leader)
      .def("current_leader", &coord::LeaderElector::current_leader);

  // Test-only: serialize a one-shard DATA_PULL request exactly as the wire
  // sees it (hostile-input tests craft out-of-range pulls without mirroring
  // the serde layout in Python).
  m.def("encode_pull_req_for_test",
        [](const std::string& dst_pool, uint64_t dst_offset, uint64_t total_len,
           const std::string& src_pool, uint64_t src_offset, uint64_t src_len) {
          ShardPlacement sp;
          sp.pool_id = src_pool;
          sp.offset = src_offset;
          sp.length = src_len;
          serde::Enc e;
          serde::put(e, dst_pool);
          serde::put(e, dst_offset);
          serde::put(e, total_len);
          serde::put(e, std::vector<ShardPlacement>{sp});
          return py::bytes(e.buf);
        });

  // Test-only: the v2 batch wire codec (batch_wire.h), one message per call.
  // Values travel as dicts so the tests can hand-build them; `msg` is one of
  // put_start2_req, put_start2_resp, get_workers2_req, get_workers2_resp,
  // upsert_start, commit_token, session_open, session_open_resp,
  // commit_token_shards, patch_start_token, patch_start_token_resp. Decoding
  // a malformed body raises PROTOCOL_ERROR.
  m.def("batch_wire_encode_for_test", [](const std::string& msg, py::dict v) {
    struct Item {
      std::string key;
      uint64_t size;
    };
    auto placements = [&] {
      wire::BatchPlacements p;
      if (v.contains("view_version"))
        p.view_version = v["view_version"].cast<uint64_t>();
      if (v.contains("token")) p.token = v["token"].cast<uint64_t>();
      p.pools = v["pools"].cast<std::vector<std::string>>();
      for (auto h : v["items"]) {
        auto it = h.cast<py::dict>();
        wire::ItemPlaces ip;
        ip.status = it["status"].cast<int32_t>();
        ip.first_place = static_cast<uint32_t>(p.places.size());
        if (it.contains("size")) ip.size = it["size"].cast<uint64_t>();
        if (it.contains("checksum"))
          ip.checksum = it["checksum"].cast<uint64_t>();
        if (it.contains("places"))
          for (auto pl : it["places"]) {
            auto t = pl.cast<std::pair<uint16_t, uint64_t>>();
            p.places.push_back({t.first, t.second});
            ++ip.ncopies;
          }
        p.items.push_back(ip);
      }
      return p;
    };
    std::string out;
    if (msg == "put_start2_req") {
      std::vector<Item> items;
      for (auto h : v["items"]) {
        auto t = h.cast<std::pair<std::string, uint64_t>>();
        items.push_back({t.first, t.second});
      }
      out = wire::encode_put_start2_request(
          items, v["cfg"].cast<PlacementConfig>(), v["want_token"].cast<bool>());
    } else if (msg == "put_start2_resp") {
      out = wire::encode_put_start2_response(placements());
    } else if (msg == "get_workers2_req") {
      out = wire::encode_get_workers2_request(
          v["keys"].cast<std::vector<std::string>>());
    } else if (msg == "get_workers2_resp") {
      out = wire::encode_get_workers2_response(placements());
    } else if (msg == "upsert_start") {
      out = wire::encode_upsert_start(v["token"].cast<uint64_t>());
    } else if (msg == "commit_token") {
      auto dg = v["digests"].cast<std::vector<uint64_t>>();
      out = wire::encode_commit_token(v["token"].cast<uint64_t>(),
                                      v["release"].cast<bool>(), dg.data(),
                                      dg.size());
    } else if (msg == "session_open") {
      std::vector<Item> items;
      for (auto h : v["items"]) {
        auto t = h.cast<std::pair<std::string, uint64_t>>();
        items.push_back({t.first, t.second});
      }
      out = wire::encode_session_open(items, v["allow_striped"].cast<bool>());
    } else if (msg == "session_open_resp") {
      out = wire::encode_session_open_response(v["token"].cast<uint64_t>());
    } else if (msg == "commit_token_shards") {
      auto od = v["obj_digests"].cast<std::vector<uint64_t>>();
      auto sd = v["shard_digests"].cast<std::vector<uint64_t>>();
      out = wire::encode_commit_token_shards(
          v["token"].cast<uint64_t>(), v["release"].cast<bool>(), od.data(),
          od.size(), sd.data(), sd.size());
    } else if (msg == "patch_start_token") {
      out = wire::encode_patch_start_token(v["token"].cast<uint64_t>());
    } else if (msg == "patch_start_token_resp") {
      out = wire::encode_patch_start_token_response(
          {v["obj_digests"].cast<std::vector<uint64_t>>(),
           v["shard_digests"].cast<std::vector<uint64_t>>()});
    } else {
      throw BlackbirdError(ErrorCode::INVALID_ARGUMENT, msg);
    }
    return py::bytes(out);
  });
  m.def("batch_wire_decode_for_test",
        [](const std::string& msg, const std::string& body, size_t nitems) {
          py::dict v;
          auto placements = [&](const wire::BatchPlacements& p, bool get) {
            v["pools"] = p.pools;
            py::list items;
            for (auto& ip : p.items) {
              py::dict it;
              it["status"] = ip.status;
              if (ip.status == 0) {
                if (get) {
                  it["size"] = ip.size;
                  it["checksum"] = ip.checksum;
                }
                py::list places;
                for (uint8_t c = 0; c < ip.ncopies; ++c)
                  places.append(py::make_tuple(p.places_of(ip)[c].pool_idx,
                                               p.places_of(ip)[c].offset));
                it["places"] = places;
              }
              items.append(it);
            }
            v["items"] = items;
          };
          if (msg == "put_start2_req") {
            auto r = unwrap(wire::decode_put_start2_request(body));
            py::list items;
            for (size_t i = 0; i < r.keys.size(); ++i)
              items.append(py::make_tuple(r.keys[i], r.sizes[i]));
            v["items"] = items;
            v["cfg"] = r.cfg;
            v["want_token"] = r.want_token != 0;
          } else if (msg == "put_start2_resp") {
            wire::BatchPlacements p;
            unwrap_void(wire::decode_put_start2_response(body, nitems, p));
            v["view_version"] = p.view_version;
            v["token"] = p.token;
            placements(p, false);
          } else if (msg == "get_workers2_req") {
            v["keys"] = unwrap(wire::decode_get_workers2_request(body));
          } else if (msg == "get_workers2_resp") {
            wire::BatchPlacements p;
            unwrap_void(wire::decode_get_workers2_response(body, nitems, p));
            placements(p, true);
          } else if (msg == "upsert_start") {
            v["token"] = unwrap(wire::decode_upsert_start(body));
          } else if (msg == "commit_token") {
            auto c = unwrap(wire::decode_commit_token(body));
            v["token"] = c.token;
            v["release"] = (c.flags & 1) != 0;
            v["digests"] = c.digests;
          } else if (msg == "session_open") {
            auto r = unwrap(wire::decode_session_open(body));
            py::list items;
            for (size_t i = 0; i < r.keys.size(); ++i)
              items.append(py::make_tuple(r.keys[i], r.sizes[i]));
            v["items"] = items;
            v["allow_striped"] = (r.flags & 1) != 0;
          } else if (msg == "session_open_resp") {
            v["token"] = unwrap(wire::decode_session_open_response(body));
          } else if (msg == "commit_token_shards") {
            auto c = unwrap(wire::decode_commit_token_shards(body));
            v["token"] = c.token;
            v["release"] = (c.flags & 1) != 0;
            v["obj_digests"] = c.obj_digests;
            v["shard_digests"] = c.shard_digests;
          } else if (msg == "patch_start_token") {
            v["token"] = unwrap(wire::decode_patch_start_token(body));
          } else if (msg == "patch_start_token_resp") {
            auto r = unwrap(wire::decode_patch_start_token_response(body));
            v["obj_digests"] = r.obj_digests;
            v["shard_digests"] = r.shard_digests;
          } else {
            throw BlackbirdError(ErrorCode::INVALID_ARGUMENT, msg);
          }
          return v;
        },
        py::arg("msg"), py::arg("body"), py::arg("nitems") = 0);

  // ------------------------------------------------------------- gpu
  auto gm = m.def_submodule("gpu");
  gm.def("available", &gpu::available);
  gm.def("device_count", &gpu::device_count);
  gm.def("digest_grid_waves", &gpu::digest_grid_waves, py::arg("total_tiles"));
  gm.def("digest_walk_depth", &gpu::digest_walk_depth);
  gm.def("checksum_cpu_tiles", [](py::buffer b, uint64_t first_tile) {
    py::buffer_info info = b.request();
    return gpu::checksum_cpu_tiles(info.ptr,
                                   static_cast<uint64_t>(info.size * info.itemsize),
                                   first_tile);
  });
  gm.def("checksum_cpu_finalize", &gpu::checksum_cpu_finalize);
  gm.def("checksum_cpu_unfinalize", &gpu::checksum_cpu_unfinalize);
  gm.def("checksum_cpu", [](py::buffer b) {
    py::buffer_info info = b.request();
    return gpu::checksum_cpu(info.ptr,
                             static_cast<uint64_t>(info.size * info.itemsize));
  });
  gm.def("sync", [] {
    py::gil_scoped_release rel;
    unwrap_void(gpu::sync());
  });
  gm.def("malloc", [](uint64_t nbytes, int device) {
    return unwrap(gpu::device_malloc(nbytes, device));
  }, py::arg("nbytes"), py::arg("device") = 0);
  gm.def("free", [](uint64_t ptr) { unwrap_void(gpu::device_free(ptr)); });
  gm.def("upload", [](uint64_t dst, py::buffer b) {
    py::buffer_info info = b.request();
    unwrap_void(gpu::upload(dst, info.ptr,
                            static_cast<uint64_t>(info.size * info.itemsize)));
  });
  gm.def("download", [](uint64_t src, uint64_t nbytes) {
    std::string out;
    out.resize(nbytes);
    unwrap_void(gpu::download(out.data(), src, nbytes));
    return py::bytes(out);
  });
  gm.def("checksum_device", [](uint64_t ptr, uint64_t nbytes, int device) {
    py::gil_scoped_release rel;
    return unwrap(gpu::checksum_sync(reinterpret_cast<const void*>(ptr), nbytes,
                                     device, nullptr));
  }, py::arg("ptr"), py::arg("nbytes"), py::arg("device") = 0);
  gm.def("checksum_device_batch",
         [](const std::vector<std::pair<uint64_t, uint64_t>>& objs, int device) {
           std::vector<const void*> ptrs;
           std::vector<uint64_t> sizes;
           for (auto& [p, s] : objs) {
             ptrs.push_back(reinterpret_cast<const void*>(p));
             sizes.push_back(s);
           }
           std::vector<uint64_t> out(objs.size());
           py::gil_scoped_release rel;
           unwrap_void(gpu::checksum_batch(ptrs.data(), sizes.data(),
                                           static_cast<uint32_t>(objs.size()),
                                           out.data(), device, nullptr));
           return out;
         }, py::arg("objs"), py::arg("device") = 0);
  using DescTuples = std::vector<std::tuple<uint64_t, uint64_t, uint64_t>>;
  auto to_put_descs = [](const DescTuples& descs) {
    std::vector<gpu::PutDesc> ds;
    for (auto& [src, dst, n] : descs)
      ds.push_back({reinterpret_cast<const void*>(src),
                    reinterpret_cast<void*>(dst), n});
    return ds;
  };
  // warm_bytes / warm_loads: gpu::WarmTail
  gm.def("fused_put", [to_put_descs](const DescTuples& descs,
                                     uint64_t warm_bytes, bool warm_loads) {
    auto ds = to_put_descs(descs);
    // poisoned: finalize(0, 0) is 0, so a digest that was never written
    // must not pass for the digest of an empty object
    std::vector<uint64_t> out(ds.size(), ~0ull);
    py::gil_scoped_release rel;
    unwrap_void(gpu::fused_put(ds.data(), static_cast<uint32_t>(ds.size()),
                               out.data(), nullptr, {warm_bytes, warm_loads}));
    return out;
  }, py::arg("descs"), py::arg("warm_bytes") = 0,
     py::arg("warm_loads") = false);
  // striped copy+digest: segs are (src, dst, nbytes, first_tile, obj) tuples;
  // returns (segment digests, object digests)
  using SegTuples =
      std::vector<std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint32_t>>;
  auto to_stripe_segs = [](const SegTuples& segs) {
    std::vector<gpu::StripeSeg> ss;
    for (auto& [src, dst, n, first_tile, obj] : segs)
      ss.push_back({reinterpret_cast<const void*>(src),
                    reinterpret_cast<void*>(dst), n, first_tile, obj});
    return ss;
  };
  gm.def("fused_stripe", [to_stripe_segs](const SegTuples& segs,
                                          const std::vector<uint64_t>& obj_sizes) {
    auto ss = to_stripe_segs(segs);
    // poisoned, as in fused_put
    std::vector<uint64_t> seg_out(ss.size(), ~0ull);
    std::vector<uint64_t> obj_out(obj_sizes.size(), ~0ull);
    py::gil_scoped_release rel;
    unwrap_void(gpu::fused_stripe(ss.data(), static_cast<uint32_t>(ss.size()),
                                  obj_sizes.data(),
                                  static_cast<uint32_t>(obj_sizes.size()),
                                  seg_out.data(), obj_out.data(), nullptr));
    return std::make_pair(seg_out, obj_out);
  }, py::arg("segs"), py::arg("obj_sizes"));
  // the argument check of fused_stripe alone (no GPU): raises INVALID_ARGUMENT
  gm.def("check_stripe_segs", [to_stripe_segs](const SegTuples& segs,
                                               const std::vector<uint64_t>& obj_sizes) {
    auto ss = to_stripe_segs(segs);
    unwrap_void(gpu::check_stripe_segs(ss.data(), static_cast<uint32_t>(ss.size()),
                                       obj_sizes.data(),
                                       static_cast<uint32_t>(obj_sizes.size())));
  }, py::arg("segs"), py::arg("obj_sizes"));
  // one copy's shard lengths → [(offset, nbytes, first_tile)], None = not fusable
  gm.def("plan_stripe", [](uint64_t obj_size, const std::vector<uint64_t>& shard_lens)
                            -> std::optional<std::vector<
                                std::tuple<uint64_t, uint64_t, uint64_t>>> {
    auto plan = gpu::plan_stripe(obj_size, shard_lens);
    if (!plan) return std::nullopt;
    std::vector<std::tuple<uint64_t, uint64_t, uint64_t>> out;
    for (const auto& p : *plan) out.emplace_back(p.offset, p.nbytes, p.first_tile);
    return out;
  }, py::arg("obj_size"), py::arg("shard_lens"));
  // in-place range patch: runs are (src, dst, nbytes, shard_tile, obj_tile,
  // shard, obj) tuples; returns (shard digests, object digests)
  using PatchTuples = std::vector<std::tuple<uint64_t, uint64_t, uint64_t,
                                             uint64_t, uint64_t, uint32_t, uint32_t>>;
  using U64s = std::vector<uint64_t>;
  auto to_patch_segs = [](const PatchTuples& segs, const U64s& shard_lens,
                          const U64s& shard_old, const U64s& obj_sizes,
                          const U64s& obj_old) {
    if (shard_lens.size() != shard_old.size() || obj_sizes.size() != obj_old.size())
      throw BlackbirdError(ErrorCode::INVALID_ARGUMENT,
                           "one old digest per shard and per object");
    std::vector<gpu::PatchSeg> ss;
    for (auto& [src, dst, n, shard_tile, obj_tile, shard, obj] : segs)
      ss.push_back({reinterpret_cast<const void*>(src),
                    reinterpret_cast<void*>(dst), n, shard_tile, obj_tile, shard,
                    obj});
    return ss;
  };
  // edges are (src, tile, lo, hi, valid, shard_tile, obj_tile, shard, obj)
  // tuples, a trailing optional argument wherever runs are taken
  using EdgeTuples =
      std::vector<std::tuple<uint64_t, uint64_t, uint32_t, uint32_t, uint32_t,
                             uint64_t, uint64_t, uint32_t, uint32_t>>;
  auto to_patch_edges = [](const EdgeTuples& edges) {
    std::vector<gpu::PatchEdge> es;
    for (auto& [src, tile, lo, hi, valid, shard_tile, obj_tile, shard, obj] : edges)
      es.push_back({reinterpret_cast<const void*>(src),
                    reinterpret_cast<void*>(tile), lo, hi, valid, shard_tile,
                    obj_tile, shard, obj});
    return es;
  };
  gm.def("fused_patch", [to_patch_segs, to_patch_edges](
                            const PatchTuples& segs, const U64s& shard_lens,
                            const U64s& shard_old, const U64s& obj_sizes,
                            const U64s& obj_old, const EdgeTuples& edges) {
    auto ss = to_patch_segs(segs, shard_lens, shard_old, obj_sizes, obj_old);
    auto es = to_patch_edges(edges);
    // poisoned, as in fused_put
    U64s shard_out(shard_lens.size(), ~0ull), obj_out(obj_sizes.size(), ~0ull);
    py::gil_scoped_release rel;
    unwrap_void(gpu::fused_patch(
        ss.data(), static_cast<uint32_t>(ss.size()), shard_lens.data(),
        shard_old.data(), static_cast<uint32_t>(shard_lens.size()),
        obj_sizes.data(), obj_old.data(), static_cast<uint32_t>(obj_sizes.size()),
        shard_out.data(), obj_out.data(), nullptr, es.data(),
        static_cast<uint32_t>(es.size())));
    return std::make_pair(shard_out, obj_out);
  }, py::arg("segs"), py::arg("shard_lens"), py::arg("shard_old"),
     py::arg("obj_sizes"), py::arg("obj_old"), py::arg("edges") = EdgeTuples{});
  gm.def("patch_walk_depth", &gpu::patch_walk_depth);
  // the argument check of fused_patch alone (no GPU): raises INVALID_ARGUMENT
  gm.def("check_patch_segs", [to_patch_segs, to_patch_edges](
                                 const PatchTuples& segs, const U64s& shard_lens,
                                 const U64s& shard_old, const U64s& obj_sizes,
                                 const U64s& obj_old, const EdgeTuples& edges) {
    auto ss = to_patch_segs(segs, shard_lens, shard_old, obj_sizes, obj_old);
    auto es = to_patch_edges(edges);
    unwrap_void(gpu::check_patch_segs(
        ss.data(), static_cast<uint32_t>(ss.size()), shard_lens.data(),
        shard_old.data(), static_cast<uint32_t>(shard_lens.size()),
        obj_sizes.data(), obj_old.data(),
        static_cast<uint32_t>(obj_sizes.size())));
    unwrap_void(gpu::check_patch_edges(
        es.data(), static_cast<uint32_t>(es.size()), ss.data(),
        static_cast<uint32_t>(ss.size()), shard_lens.data(),
        static_cast<uint32_t>(shard_lens.size()), obj_sizes.data(),
        static_cast<uint32_t>(obj_sizes.size())));
  }, py::arg("segs"), py::arg("shard_lens"), py::arg("shard_old"),
     py::arg("obj_sizes"), py::arg("obj_old"), py::arg("edges") = EdgeTuples{});
  // the edge rules alone, against runs that passed the check above
  gm.def("check_patch_edges", [to_patch_edges](const EdgeTuples& edges,
                                               const PatchTuples& segs,
                                               const U64s& shard_lens,
                                               const U64s& obj_sizes) {
    std::vector<gpu::PatchSeg> ss;
    for (auto& [src, dst, n, shard_tile, obj_tile, shard, obj] : segs)
      ss.push_back({reinterpret_cast<const void*>(src),
                    reinterpret_cast<void*>(dst), n, shard_tile, obj_tile, shard,
                    obj});
    auto es = to_patch_edges(edges);
    unwrap_void(gpu::check_patch_geometry(
        ss.data(), static_cast<uint32_t>(ss.size()), shard_lens.data(),
        static_cast<uint32_t>(shard_lens.size()), obj_sizes.data(),
        static_cast<uint32_t>(obj_sizes.size())));
    unwrap_void(gpu::check_patch_edges(
        es.data(), static_cast<uint32_t>(es.size()), ss.data(),
        static_cast<uint32_t>(ss.size()), shard_lens.data(),
        static_cast<uint32_t>(shard_lens.size()), obj_sizes.data(),
        static_cast<uint32_t>(obj_sizes.size())));
  }, py::arg("edges"), py::arg("segs"), py::arg("shard_lens"),
     py::arg("obj_sizes"));
  // a byte range of one copy → [(shard, shard_off, obj_off, nbytes)];
  // plan_patch: None = not patchable in place; range_pieces: None = the range
  // leaves the object or the lengths do not add up
  using PieceTuples =
      std::vector<std::tuple<uint32_t, uint64_t, uint64_t, uint64_t>>;
  auto to_piece_tuples = [](const std::optional<std::vector<gpu::RangePiece>>& plan)
      -> std::optional<PieceTuples> {
    if (!plan) return std::nullopt;
    PieceTuples out;
    for (const auto& p : *plan)
      out.emplace_back(p.shard, p.shard_off, p.obj_off, p.nbytes);
    return out;
  };
  gm.def("plan_patch", [to_piece_tuples](uint64_t obj_size, const U64s& shard_lens,
                                         uint64_t offset, uint64_t length) {
    return to_piece_tuples(gpu::plan_patch(obj_size, shard_lens, offset, length));
  }, py::arg("obj_size"), py::arg("shard_lens"), py::arg("offset"),
     py::arg("length"));
  // the same at byte granularity: (runs, edges), runs as plan_patch's pieces,
  // edges as (shard, shard_tile, obj_tile, lo, hi, valid, src_off); None =
  // plan_stripe refuses the copy or the range leaves the object
  gm.def("plan_patch_bytes", [to_piece_tuples](uint64_t obj_size,
                                               const U64s& shard_lens,
                                               uint64_t offset, uint64_t length)
      -> std::optional<std::pair<
          PieceTuples, std::vector<std::tuple<uint32_t, uint64_t, uint64_t, uint32_t,
                                              uint32_t, uint32_t, uint64_t>>>> {
    auto plan = gpu::plan_patch_bytes(obj_size, shard_lens, offset, length);
    if (!plan) return std::nullopt;
    std::vector<std::tuple<uint32_t, uint64_t, uint64_t, uint32_t, uint32_t,
                           uint32_t, uint64_t>> edges;
    for (const auto& e : plan->edges)
      edges.emplace_back(e.shard, e.shard_tile, e.obj_tile, e.lo, e.hi, e.valid,
                         e.src_off);
    return std::make_pair(*to_piece_tuples(plan->runs), edges);
  }, py::arg("obj_size"), py::arg("shard_lens"), py::arg("offset"),
     py::arg("length"));
  gm.def("range_pieces", [to_piece_tuples](uint64_t obj_size, const U64s& shard_lens,
                                           uint64_t offset, uint64_t length) {
    return to_piece_tuples(gpu::range_pieces(obj_size, shard_lens, offset, length));
  }, py::arg("obj_size"), py::arg("shard_lens"), py::arg("offset"),
     py::arg("length"));
  // one FusedPutPlan, replayed `steps` times: one digest list per step.
  // before_step(k), when given, runs before replay k, as in
  // fused_stripe_plan below.
  gm.def("fused_put_plan",
         [to_put_descs](const DescTuples& descs, int steps, int device,
                        uint64_t warm_bytes, bool warm_loads,
                        py::object before_step) {
           auto ds = to_put_descs(descs);
           std::vector<std::vector<uint64_t>> out(
               steps, std::vector<uint64_t>(ds.size()));
           gpu::FusedPutPlan plan;
           {
             py::gil_scoped_release rel;
             unwrap_void(plan.build(ds.data(), static_cast<uint32_t>(ds.size()),
                                    device, {warm_bytes, warm_loads}));
           }
           for (int k = 0; k < steps; ++k) {
             if (!before_step.is_none()) before_step(k);
             py::gil_scoped_release rel;
             unwrap_void(plan.run(out[k].data()));
           }
           return out;
         }, py::arg("descs"), py::arg("steps"), py::arg("device") = 0,
         py::arg("warm_bytes") = 0, py::arg("warm_loads") = false,
         py::arg("before_step") = py::none());
  // one FusedStripePlan, replayed `steps` times: one (segment digests, object
  // digests) pair per step, poisoned before each run as in fused_stripe.
  // before_step(k), when given, runs before replay k (a test rewrites the
  // source there).
  gm.def("fused_stripe_plan",
         [to_stripe_segs](const SegTuples& segs,
                          const std::vector<uint64_t>& obj_sizes, int steps,
                          int device, py::object before_step) {
           auto ss = to_stripe_segs(segs);
           std::vector<std::pair<std::vector<uint64_t>, std::vector<uint64_t>>>
               out;
           gpu::FusedStripePlan plan;
           {
             py::gil_scoped_release rel;
             unwrap_void(plan.build(ss.data(), static_cast<uint32_t>(ss.size()),
                                    obj_sizes.data(),
                                    static_cast<uint32_t>(obj_sizes.size()),
                                    device));
           }
           for (int k = 0; k < steps; ++k) {
             if (!before_step.is_none()) before_step(k);
             out.emplace_back(std::vector<uint64_t>(ss.size(), ~0ull),
                              std::vector<uint64_t>(obj_sizes.size(), ~0ull));
             py::gil_scoped_release rel;
             unwrap_void(plan.run(out.back().first.data(),
                                  out.back().second.data()));
           }
           return out;
         }, py::arg("segs"), py::arg("obj_sizes"), py::arg("steps"),
         py::arg("device") = 0, py::arg("before_step") = py::none());
  // one FusedPatchPlan, replayed `steps` times: one (shard digests, object
  // digests) pair per step, poisoned before each run. Step k's old digests
  // are step k-1's outputs; the first step takes the given ones.
  // before_step(k), when given, runs before replay k.
  gm.def("fused_patch_plan",
         [to_patch_segs, to_patch_edges](
             const PatchTuples& segs, const U64s& shard_lens,
             const U64s& obj_sizes, U64s shard_old, U64s obj_old, int steps,
             int device, py::object before_step, const EdgeTuples& edges) {
           auto ss = to_patch_segs(segs, shard_lens, shard_old, obj_sizes, obj_old);
           auto es = to_patch_edges(edges);
           std::vector<std::pair<U64s, U64s>> out;
           gpu::FusedPatchPlan plan;
           {
             py::gil_scoped_release rel;
             unwrap_void(plan.build(ss.data(), static_cast<uint32_t>(ss.size()),
                                    shard_lens.data(),
                                    static_cast<uint32_t>(shard_lens.size()),
                                    obj_sizes.data(),
                                    static_cast<uint32_t>(obj_sizes.size()),
                                    device, es.data(),
                                    static_cast<uint32_t>(es.size())));
           }
           for (int k = 0; k < steps; ++k) {
             if (!before_step.is_none()) before_step(k);
             out.emplace_back(U64s(shard_lens.size(), ~0ull),
                              U64s(obj_sizes.size(), ~0ull));
             {
               py::gil_scoped_release rel;
               unwrap_void(plan.run(shard_old.data(), obj_old.data(),
                                    out.back().first.data(),
                                    out.back().second.data()));
             }
             shard_old = out.back().first;
             obj_old = out.back().second;
           }
           return out;
         }, py::arg("segs"), py::arg("shard_lens"), py::arg("obj_sizes"),
         py::arg("shard_old"), py::arg("obj_old"), py::arg("steps"),
         py::arg("device") = 0, py::arg("before_step") = py::none(),
         py::arg("edges") = EdgeTuples{});
  gm.def("batched_copy",
         [](const std::vector<std::tuple<uint64_t, uint64_t, uint64_t>>& descs) {
           std::vector<gpu::CopyDesc> ds;
           for (auto& [src, dst, n] : descs)
             ds.push_back({reinterpret_cast<const void*>(src),
                           reinterpret_cast<void*>(dst), n});
           py::gil_scoped_release rel;
           unwrap_void(gpu::batched_copy(ds.data(),
                                         static_cast<uint32_t>(ds.size()), nullptr));
           unwrap_void(gpu::sync());
         });
  gm.def("fill_pattern", [](uint64_t ptr, uint64_t nbytes, uint64_t seed) {
    py::gil_scoped_release rel;
    unwrap_void(gpu::fill_pattern(reinterpret_cast<void*>(ptr), nbytes, seed, nullptr));
    unwrap_void(gpu::sync());
  }, py::arg("ptr"), py::arg("nbytes"), py::arg("seed") = 0);
  gm.def("verify_pattern", [](uint64_t ptr, uint64_t nbytes, uint64_t seed) {
    py::gil_scoped_release rel;
    return unwrap(gpu::verify_pattern(reinterpret_cast<const void*>(ptr), nbytes,
                                      seed, nullptr));
  }, py::arg("ptr"), py::arg("nbytes"), py::arg("seed") = 0);
  gm.def("mfma_i8_probe", [](py::buffer a, py::buffer b, int device) {
    py::buffer_info ia = a.request(), ib = b.request();
    if (ia.size * ia.itemsize != 1024 || ib.size * ib.itemsize != 1024)
      throw std::runtime_error("A and B must be 1024 bytes (32x32 i8)");
    std::vector<int32_t> c(1024);
    unwrap_void(gpu::mfma_i8_probe(static_cast<const int8_t*>(ia.ptr),
                                   static_cast<const int8_t*>(ib.ptr), c.data(),
                                   device));
    return c;
  }, py::arg("a"), py::arg("b"), py::arg("device") = 0);

  bind_store(m);
}
