// bb_selftest — native concurrency self-test, built with -fsanitize=thread
// by scripts/run_tsan.sh (the reference had no sanitizer coverage at all,
// SURVEY §5.2). Exercises the lock-heavy subsystems from many threads:
// allocators under churn, the coordination store with watches firing during
// mutation, a keystone put/get/remove storm with maintenance passes, the
// client placement cache with session bindings racing recorders and erasers,
// and the clients' batch fan-out.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "blackbird/allocation/pool_allocator.h"
#include "blackbird/allocation/range_allocator.h"
#include "blackbird/client/batch_util.h"
#include "blackbird/client/placement_cache.h"
#include "blackbird/coord/coord.h"
#include "blackbird/keystone/keystone_rpc.h"
#include "blackbird/keystone/keystone_service.h"
#include "blackbird/rpc/methods.h"
#include "blackbird/rpc/rpc.h"

using namespace blackbird;

namespace {

int failures = 0;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "CHECK failed at %s:%d: %s\n", __FILE__,      \
                   __LINE__, #cond);                                     \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

void pool_allocator_storm() {
  PoolAllocator a(256ull << 20);
  std::vector<std::thread> ts;
  for (int t = 0; t < 8; ++t) {
    ts.emplace_back([&a] {
      std::vector<std::pair<uint64_t, uint64_t>> mine;
      for (int i = 0; i < 500; ++i) {
        uint64_t size = (i % 3 == 0) ? 65536 : 7000 + i;
        auto r = a.allocate(size);
        if (r.ok()) mine.emplace_back(r.value(), size);
        if (mine.size() > 32) {
          auto [off, sz] = mine.back();
          mine.pop_back();
          CHECK(a.free(off, sz).ok());
        }
      }
      for (auto [off, sz] : mine) CHECK(a.free(off, sz).ok());
    });
  }
  for (auto& t : ts) t.join();
  CHECK(a.used() == 0);
}

void range_allocator_storm() {
  RangeAllocator ra;
  for (int i = 0; i < 8; ++i) {
    MemoryPool p;
    p.pool_id = "p" + std::to_string(i);
    p.worker_id = "w" + std::to_string(i % 4);
    p.storage_class = StorageClass::RAM_GPU;
    p.size = 1ull << 30;
    ra.upsert_pool(p);
  }
  std::vector<std::thread> ts;
  for (int t = 0; t < 8; ++t) {
    ts.emplace_back([&ra, t] {
      PlacementConfig cfg;
      cfg.replication = 1 + (t % 2);
      for (int i = 0; i < 300; ++i) {
        std::string key = "t" + std::to_string(t) + "k" + std::to_string(i);
        auto r = ra.allocate(key, 1 << 20, cfg);
        CHECK(r.ok());
        if (i % 2 == 0) CHECK(ra.free(key).ok());
      }
      for (int i = 1; i < 300; i += 2)
        ra.free("t" + std::to_string(t) + "k" + std::to_string(i));
    });
  }
  // membership churn concurrent with allocation
  ts.emplace_back([&ra] {
    for (int i = 0; i < 50; ++i) {
      MemoryPool p;
      p.pool_id = "extra";
      p.worker_id = "wx";
      p.storage_class = StorageClass::RAM_CPU;
      p.size = 1 << 26;
      ra.upsert_pool(p);
      ra.remove_pool("extra");
    }
  });
  for (auto& t : ts) t.join();
  CHECK(ra.stats().total_used == 0);
}

void coord_storm() {
  auto store = std::make_shared<coord::CoordStore>();
  coord::InProcCoord c(store);
  std::atomic<int> events{0};
  auto w = c.watch_prefix("/storm/", [&](const coord::WatchEvent&) { ++events; });
  CHECK(w.ok());
  std::vector<std::thread> ts;
  for (int t = 0; t < 6; ++t) {
    ts.emplace_back([&c, t] {
      for (int i = 0; i < 400; ++i) {
        std::string k = "/storm/t" + std::to_string(t) + "/" + std::to_string(i);
        CHECK(c.put(k, "v", i % 4 == 0 ? 5 : 0).ok());
        if (i % 3 == 0) c.del(k);
        if (i % 7 == 0) c.get_prefix("/storm/");
        if (i % 11 == 0) c.cas("/storm/lock", "", true, "t" + std::to_string(t), 10);
      }
    });
  }
  for (auto& t : ts) t.join();
  c.unwatch(w.value());
  CHECK(events.load() > 0);
}

void keystone_storm() {
  KeystoneConfig cfg;
  cfg.gc_interval_ms = 20;  // maintenance races with the mutation storm
  auto coord = std::make_shared<coord::InProcCoord>(
      std::make_shared<coord::CoordStore>());
  KeystoneService ks(cfg, coord);
  CHECK(ks.initialize().ok());
  CHECK(ks.start().ok());
  for (int i = 0; i < 4; ++i) {
    MemoryPool p;
    p.pool_id = "kp" + std::to_string(i);
    p.worker_id = "kw" + std::to_string(i);
    p.storage_class = StorageClass::RAM_CPU;
    p.size = 1ull << 28;
    ks.register_pool(p);
  }
  std::vector<std::thread> ts;
  for (int t = 0; t < 6; ++t) {
    ts.emplace_back([&ks, t] {
      PlacementConfig pc;
      pc.ttl_ms = (t % 2) ? 15 : 0;  // half the objects expire mid-storm
      for (int i = 0; i < 300; ++i) {
        std::string key = "s" + std::to_string(t) + "o" + std::to_string(i);
        auto r = ks.put_start(key, 65536, pc);
        if (!r.ok()) continue;
        ks.put_complete(key, 1);
        ks.object_exists(key);
        ks.get_workers(key);
        if (i % 2 == 0) ks.remove_object(key);
        if (i % 50 == 0) ks.get_cluster_stats();
      }
    });
  }
  for (auto& t : ts) t.join();
  ks.remove_all_objects();
  ks.stop();
  CHECK(ks.get_cluster_stats().total_used == 0);
}

struct PutCompleteListMsg {
  std::vector<PutCompleteRequest> reqs;
  BB_FIELDS(reqs)
};

// Mirrors the flagship bench's control-plane pattern over the REAL wire:
// v2 batch put_start with replace=true cycling the same key space, batch
// complete, v2 get_workers — through KeystoneRpc + RpcClient, then a
// worker-death cleanup with thousands of live objects.
void v2_replace_storm() {
  KeystoneConfig cfg;
  cfg.listen_address = "127.0.0.1:0";
  cfg.gc_interval_ms = 50;
  auto store = std::make_shared<coord::CoordStore>();
  auto coord = std::make_shared<coord::InProcCoord>(store);
  auto ks = std::make_shared<KeystoneService>(cfg, coord);
  CHECK(ks->initialize().ok());
  CHECK(ks->start().ok());
  KeystoneServer krpc(ks);
  CHECK(krpc.start().ok());
  for (int i = 0; i < 2; ++i) {
    MemoryPool p;
    p.pool_id = "vp" + std::to_string(i);
    p.worker_id = "vw" + std::to_string(i);
    p.storage_class = StorageClass::RAM_CPU;
    p.size = 1ull << 28;
    ks->register_pool(p);
  }
  const int kObjects = 4096;
  std::vector<std::thread> lanes;
  for (int L = 0; L < 2; ++L) {
    lanes.emplace_back([&, L] {
      rpc::RpcClient c;
      CHECK(c.connect(krpc.endpoint()).ok());
      for (int step = 0; step < 8; ++step) {
        // BATCH_PUT_START2: uniform size, replace=true
        serde::Enc req;
        req.num<uint32_t>(kObjects);
        req.num<uint64_t>(16384);  // uniform
        for (int i = 0; i < kObjects; ++i)
          req.str("L" + std::to_string(L) + "o" + std::to_string(i));
        PlacementConfig pc;
        pc.replace = true;
        serde::put(req, pc);
        auto resp = c.call_raw(rpc::methods::BATCH_PUT_START2, req.buf, 30000);
        CHECK(resp.ok());
        // BATCH_PUT_COMPLETE
        PutCompleteListMsg completes;
        for (int i = 0; i < kObjects; ++i)
          completes.reqs.push_back(
              {"L" + std::to_string(L) + "o" + std::to_string(i),
               0x1234ULL + i});
        auto cr = c.call_raw(rpc::methods::BATCH_PUT_COMPLETE,
                             serde::to_bytes(completes), 30000);
        CHECK(cr.ok());
        // BATCH_GET_WORKERS2
        serde::Enc greq;
        greq.num<uint32_t>(kObjects);
        for (int i = 0; i < kObjects; ++i)
          greq.str("L" + std::to_string(L) + "o" + std::to_string(i));
        auto gr = c.call_raw(rpc::methods::BATCH_GET_WORKERS2, greq.buf, 30000);
        CHECK(gr.ok());
      }
      c.close();
    });
  }
  for (auto& t : lanes) t.join();
  // worker death with thousands of live objects (the bench teardown shape)
  ks->remove_worker("vw0");
  ks->remove_worker("vw1");
  krpc.stop();
  ks->stop();
}

// Replication under concurrency: writers hammer the primary through
// multi-endpoint clients while the standby mirrors; the primary dies
// mid-storm, the standby promotes, and the same clients keep writing.
void coord_repl_storm() {
  auto store_a = std::make_shared<coord::CoordStore>();
  auto server_a = std::make_unique<coord::CoordServer>(store_a);
  CHECK(server_a->start("127.0.0.1", 0).ok());
  auto store_b = std::make_shared<coord::CoordStore>();
  coord::CoordServer server_b(store_b);
  CHECK(server_b.start("127.0.0.1", 0).ok());
  const std::string ep_a = server_a->endpoint();
  const std::string ep_b = server_b.endpoint();
  coord::CoordFollower follower(store_b, &server_b, ep_a, 300);
  CHECK(follower.start().ok());

  std::atomic<bool> stop_writers{false};
  std::atomic<int> ok_writes{0};
  std::vector<std::thread> ts;
  for (int t = 0; t < 4; ++t) {
    ts.emplace_back([&, t] {
      coord::CoordClient c;
      CHECK(c.connect(ep_a + "," + ep_b).ok());
      for (int i = 0; i < 400 && !stop_writers.load(); ++i) {
        std::string k = "/repl/t" + std::to_string(t) + "/" + std::to_string(i);
        if (c.put(k, "v", i % 3 == 0 ? 50 : 0).ok()) ++ok_writes;
        if (i % 5 == 0) (void)c.get(k);
        if (i == 150 && t == 0) {
          server_a->stop();  // primary dies mid-storm
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
      }
      c.close();
    });
  }
  for (auto& t : ts) t.join();
  // follower must have promoted and the standby must be serving writes
  for (int i = 0; i < 100 && !follower.promoted(); ++i)
    std::this_thread::sleep_for(std::chrono::milliseconds(50));
  CHECK(follower.promoted());
  CHECK(!server_b.read_only());
  CHECK(ok_writes.load() > 0);
  {
    coord::CoordClient c;
    CHECK(c.connect(ep_b).ok());
    CHECK(c.put("/repl/final", "done", 0).ok());
    auto v = c.get("/repl/final");
    CHECK(v.ok() && v.value() == "done");
    c.close();
  }
  follower.stop();
  server_b.stop();
  server_a.reset();
}

// Session bindings against concurrent recorders and an eraser: a digest a
// binding reads (or finds it may refresh) is always one some recorder wrote
// for that very key — never a freed or foreign slot. Digests are
// (key index + 1) << 32 | counter, so the check is exact.
void placement_cache_storm() {
  using PC = PlacementCache;
  constexpr uint32_t kKeys = 64;
  PC cache;
  cache.set_enabled(true);
  std::vector<ObjectKey> keys;
  for (uint32_t k = 0; k < kKeys; ++k) keys.push_back("pc" + std::to_string(k));
  PC::KeyList all;
  for (const auto& k : keys) all.push_back(&k);
  auto digest_of = [](uint32_t k, uint32_t n) {
    return (uint64_t{k} + 1) << 32 | n;
  };
  auto record_all = [&](uint32_t n, bool move) {
    std::vector<PC::Put> puts;
    for (uint32_t k = 0; k < kKeys; ++k)
      puts.push_back({keys[k], {"pool", (move ? n : 0) * 4096ull + k, 4096,
                                digest_of(k, n)}});
    return puts;
  };
  // recorders write counters 1..400, binders 1000+t, refreshes 2000+t
  auto written = [](uint32_t k, uint64_t d) {
    const uint64_t n = d & 0xffffffffu;
    return d >> 32 == k + 1 && ((n >= 1 && n <= 400) || n == 1000 ||
                                n == 1001 || n == 2000 || n == 2001);
  };
  std::atomic<bool> stop{false};
  std::atomic<uint64_t> reads{0};
  std::vector<std::thread> ts;
  for (int mover = 0; mover < 2; ++mover)
    ts.emplace_back([&, mover] {
      for (uint32_t n = 1; n <= 400; ++n)
        cache.record(record_all(n, mover == 1 && n % 8 == 0));
    });
  ts.emplace_back([&] {
    for (uint32_t n = 0; n < 400; ++n) {
      if (n % 16 == 0) cache.erase({&keys[n % kKeys], &keys[(n + 7) % kKeys]});
      std::this_thread::yield();
    }
  });
  for (int t = 0; t < 2; ++t)
    ts.emplace_back([&, t] {
      std::vector<uint64_t> got(kKeys), fresh(kKeys);
      while (!stop.load()) {
        auto b = cache.record(record_all(1000 + t, false), &all);
        CHECK(b.bound());
        for (int i = 0; i < 50 && cache.read_digests(b, got.data(), kKeys); ++i) {
          for (uint32_t k = 0; k < kKeys; ++k) {
            CHECK(written(k, got[k]));
            fresh[k] = digest_of(k, 2000 + t);
          }
          cache.refresh_digests(b, fresh.data());
          ++reads;
        }
      }
    });
  for (size_t i = 0; i < 3; ++i) ts[i].join();
  stop.store(true);
  for (size_t i = 3; i < ts.size(); ++i) ts[i].join();
  std::printf("  %llu verified digest reads\n",
              static_cast<unsigned long long>(reads.load()));

  // the size cap: one bulk record past kMaxEntries empties the cache and
  // ends the bindings taken before it
  auto b = cache.record(record_all(1, false), &all);
  std::vector<uint64_t> got(kKeys);
  CHECK(b.bound() && cache.read_digests(b, got.data(), kKeys));
  for (uint32_t k = 0; k < kKeys; ++k) CHECK(got[k] == digest_of(k, 1));
  std::vector<ObjectKey> many;
  many.reserve(PC::kMaxEntries + 1);
  for (size_t i = 0; i <= PC::kMaxEntries; ++i)
    many.push_back("bulk" + std::to_string(i));
  std::vector<PC::Put> bulk;
  bulk.reserve(many.size());
  for (const auto& k : many) bulk.push_back({k, {"pool", 0, 1, 1}});
  cache.record(bulk);
  CHECK(!cache.enabled_and_nonempty());
  CHECK(!cache.valid(b));
  CHECK(!cache.find(keys[0]));
}

// The batch fan-out from several callers at once, as pipelined batches do:
// every index of every call runs exactly once, on at most `threads` threads,
// and all of it is visible to the caller when the call returns.
void fan_out_storm() {
  std::vector<std::thread> ts;
  for (int caller = 0; caller < 4; ++caller)
    ts.emplace_back([caller] {
      for (size_t n : {size_t{0}, size_t{1}, size_t{3}, size_t{257}}) {
        const int threads = 1 + caller;
        std::vector<int> hits(n, 0);  // plain ints: each index has one writer
        std::vector<int> per_thread(threads, 0);
        fan_out_threads(n, threads, [&](int t, auto& next) {
          CHECK(t >= 0 && t < threads);
          for (size_t i; next(i);) {
            ++hits[i];
            ++per_thread[t];
          }
        });
        size_t total = 0;
        for (int c : per_thread) total += c;
        CHECK(total == n);
        for (int h : hits) CHECK(h == 1);
        std::vector<size_t> seen(n, SIZE_MAX);
        fan_out(n, threads, [&](size_t i) { seen[i] = i; });
        for (size_t i = 0; i < n; ++i) CHECK(seen[i] == i);
      }
    });
  for (auto& t : ts) t.join();
}

}  // namespace

int main() {
  std::printf("pool_allocator_storm...\n");
  pool_allocator_storm();
  std::printf("range_allocator_storm...\n");
  range_allocator_storm();
  std::printf("coord_storm...\n");
  coord_storm();
  std::printf("keystone_storm...\n");
  keystone_storm();
  std::printf("v2_replace_storm...\n");
  v2_replace_storm();
  std::printf("coord_repl_storm...\n");
  coord_repl_storm();
  std::printf("placement_cache_storm...\n");
  placement_cache_storm();
  std::printf("fan_out_storm...\n");
  fan_out_storm();
  if (failures) {
    std::printf("SELFTEST FAILED (%d checks)\n", failures);
    return 1;
  }
  std::printf("SELFTEST OK\n");
  return 0;
}
