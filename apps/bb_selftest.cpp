// bb_selftest — native concurrency self-test, built with -fsanitize=thread
// by scripts/run_tsan.sh (the reference had no sanitizer coverage at all,
// SURVEY §5.2). Exercises the lock-heavy subsystems from many threads:
// allocators under churn, the coordination store with watches firing during
// mutation, a keystone put/get/remove storm with maintenance passes, the
// client placement cache with session bindings racing recorders and erasers,
// and the clients' batch fan-out.
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "blackbird/allocation/pool_allocator.h"
#include "blackbird/allocation/range_allocator.h"
#include "blackbird/client/batch_util.h"
#include "blackbird/client/placement_cache.h"
#include "blackbird/client/pool_mapper.h"
#include "blackbird/coord/coord.h"
#include "blackbird/keystone/keystone_rpc.h"
#include "blackbird/keystone/keystone_service.h"
#include "blackbird/rpc/messages.h"
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

// ---- keystone_transitions: the object state machine, one table per
// transition. Deterministic and single-threaded: every route into a
// transition must give the same answer for the same prior state. Each cell
// prints one row (the rows are what profiles/keystone_transitions_checks.md
// records).

constexpr uint64_t kObj = 65536;

std::unique_ptr<KeystoneService> table_keystone() {
  KeystoneConfig cfg;
  cfg.gc_interval_ms = 100000;  // no maintenance pass inside a table
  auto ks = std::make_unique<KeystoneService>(
      cfg, std::make_shared<coord::InProcCoord>(
               std::make_shared<coord::CoordStore>()));
  CHECK(ks->initialize().ok());
  CHECK(ks->start().ok());
  for (int i = 0; i < 4; ++i) {
    MemoryPool p;
    p.pool_id = "tp" + std::to_string(i);
    p.worker_id = "tw" + std::to_string(i);
    p.storage_class = StorageClass::RAM_CPU;
    p.size = 1ull << 28;
    ks->register_pool(p);
  }
  return ks;
}

int32_t code_of(ErrorCode c) { return static_cast<int32_t>(c); }

bool same_placement(const std::vector<CopyPlacement>& a,
                    const std::vector<CopyPlacement>& b) {
  if (a.size() != b.size()) return false;
  for (size_t c = 0; c < a.size(); ++c)
    if (a[c].shards != b[c].shards) return false;  // pool, offset, length
  return true;
}

enum Prior { ABSENT, PENDING, SAME, OTHER_SIZE, OTHER_REPL, EXPIRED, kPriors };
enum Route { PUT_START, BATCH_OF_1, UNIFORM_8, NON_UNIFORM, kRoutes };
const char* const kPriorName[] = {"absent",     "pending",    "same",
                                  "other_size", "other_repl", "expired"};
const char* const kRouteName[] = {"put_start", "batch_of_1", "uniform_8",
                                  "non_uniform"};

struct Admitted {
  int32_t status = 0;
  size_t copies = 0, shards = 0;
  bool same_place = false;  // returned placement == the prior one
  bool erased = false;      // the prior meta was dropped (sessions went stale)
  uint64_t used = 0;        // total_used minus the batch's filler items
  int32_t get_code = 0;     // get_workers afterwards
  bool operator==(const Admitted& o) const {
    return status == o.status && copies == o.copies && shards == o.shards &&
           same_place == o.same_place && erased == o.erased &&
           used == o.used && get_code == o.get_code;
  }
};

// `key`/`size` through one route; fillers ride along in the batch routes
BatchPutStartItem admit_via(KeystoneService& ks, Route route,
                            const ObjectKey& key, uint64_t size, bool replace,
                            uint64_t* filler_bytes) {
  PlacementConfig pc;
  pc.replace = replace;
  *filler_bytes = 0;
  BatchPutStartItem item;
  if (route == PUT_START) {
    auto r = ks.put_start(key, size, pc);
    item.status = code_of(r.code());
    if (r.ok()) item.copies = r.value().copies;
    return item;
  }
  std::vector<PutStartRequest> reqs;
  size_t at = 0;
  if (route == BATCH_OF_1) {
    reqs.push_back({key, size, pc});
  } else if (route == UNIFORM_8) {
    for (int i = 0; i < 8; ++i)
      reqs.push_back({"filler" + std::to_string(i), kObj, pc});
    at = 3;
    reqs[at] = {key, size, pc};
    *filler_bytes = 7 * kObj;
  } else {
    PlacementConfig other = pc;
    other.ttl_ms = 1000000;  // a second TTL: the batch is not uniform
    reqs.push_back({key, size, pc});
    reqs.push_back({"filler", kObj, other});
    *filler_bytes = kObj;
  }
  auto resp = ks.batch_put_start(reqs);
  CHECK(resp.items.size() == reqs.size());
  for (size_t i = 0; i < resp.items.size(); ++i)
    if (i != at) CHECK(resp.items[i].status == 0);
  return resp.items[at];
}

Admitted admission_cell(Prior prior, bool replace, Route route) {
  auto ks = table_keystone();
  const ObjectKey key = "k";
  PlacementConfig pc;
  if (prior == OTHER_REPL) pc.replication = 2;
  if (prior == EXPIRED) pc.ttl_ms = 5;
  std::vector<CopyPlacement> before;
  uint64_t token = 0;
  if (prior != ABSENT) {
    auto r = ks->put_start(key, prior == OTHER_SIZE ? 2 * kObj : kObj, pc);
    CHECK(r.ok());
    before = r.value().copies;
    if (prior != PENDING) CHECK(ks->put_complete(key, 7).ok());
    // a session on the prior object goes stale exactly when its meta is
    // erased; an in-place upsert keeps it current
    token = ks->create_put_session({{key, 0, pc}});
    CHECK(token != 0);
    if (prior == EXPIRED)
      std::this_thread::sleep_for(std::chrono::milliseconds(12));
  }
  uint64_t filler = 0;
  auto item = admit_via(*ks, route, key, kObj, replace, &filler);
  Admitted a;
  a.status = item.status;
  a.copies = item.copies.size();
  for (const auto& c : item.copies) a.shards += c.shards.size();
  a.same_place = item.status == 0 && same_placement(item.copies, before);
  a.used = ks->get_cluster_stats().total_used - filler;
  a.get_code = code_of(ks->get_workers(key).code());
  if (token)
    a.erased = ks->upsert_start_token(token).code() == ErrorCode::SESSION_STALE;
  ks->stop();
  std::printf("  admission %-10s replace=%d %-11s status=%d copies=%zu "
              "shards=%zu same_place=%d erased=%d used=%llu get=%d\n",
              kPriorName[prior], replace, kRouteName[route], a.status,
              a.copies, a.shards, a.same_place, a.erased,
              static_cast<unsigned long long>(a.used), a.get_code);
  return a;
}

void admission_table() {
  const int32_t exists = code_of(ErrorCode::OBJECT_EXISTS);
  const int32_t pending = code_of(ErrorCode::OBJECT_NOT_COMMITTED);
  //                     status copies shards same   erased used      get
  const Admitted fresh    {0,      1, 1, false, false, kObj,     pending};
  const Admitted replaced {0,      1, 1, false, true,  kObj,     pending};
  const Admitted in_place {0,      1, 1, true,  false, kObj,     pending};
  const Admitted kept     {exists, 0, 0, false, false, kObj,     0};
  const Admitted kept_big {exists, 0, 0, false, false, 2 * kObj, 0};
  const Admitted kept_pend{exists, 0, 0, false, false, kObj,     pending};
  // expected[prior][replace]
  const Admitted expected[kPriors][2] = {
      /* absent     */ {fresh, fresh},
      /* pending    */ {kept_pend, replaced},
      /* same       */ {kept, in_place},
      /* other_size */ {kept_big, replaced},
      /* other_repl */ {kept_big, replaced},
      /* expired    */ {replaced, in_place},
  };
  for (int p = 0; p < kPriors; ++p)
    for (int replace = 0; replace < 2; ++replace)
      for (int r = 0; r < kRoutes; ++r) {
        auto got = admission_cell(static_cast<Prior>(p), replace,
                                  static_cast<Route>(r));
        Admitted want = expected[p][replace];
        // a dropped range may be handed out again at once: equal placement
        // proves an in-place upsert only together with erased == false
        if (want.erased) want.same_place = got.same_place;
        CHECK(got == want);
      }
  // malformed requests: refused on every route, nothing allocated
  for (int r = 0; r < kRoutes; ++r)
    for (int zero_size = 0; zero_size < 2; ++zero_size) {
      auto ks = table_keystone();
      uint64_t filler = 0;
      auto item = admit_via(*ks, static_cast<Route>(r),
                            zero_size ? "k" : "", zero_size ? 0 : kObj, false,
                            &filler);
      const uint64_t used = ks->get_cluster_stats().total_used - filler;
      ks->stop();
      std::printf("  admission %-10s replace=0 %-11s status=%d copies=%zu "
                  "used=%llu\n",
                  zero_size ? "zero_size" : "empty_key",
                  kRouteName[r], item.status, item.copies.size(),
                  static_cast<unsigned long long>(used));
      CHECK(item.status == code_of(ErrorCode::INVALID_ARGUMENT));
      CHECK(item.copies.empty());
      CHECK(used == 0);
    }
}

enum CommitRoute { PUT_COMPLETE, BATCH_COMPLETE, TOKEN, kCommitRoutes };
const char* const kCommitName[] = {"put_complete", "batch_put_complete",
                                   "commit_token"};

int32_t complete_via(KeystoneService& ks, CommitRoute route,
                     const ObjectKey& key, uint64_t checksum,
                     const std::vector<std::vector<uint64_t>>& sd = {}) {
  if (route == PUT_COMPLETE)
    return code_of(ks.put_complete(key, checksum, sd).code());
  auto st = ks.batch_put_complete({{key, checksum, sd}});
  CHECK(st.size() == 1);
  return st.empty() ? -1 : st[0];
}

// committed, carrying `checksum`, with `digests` on the shards of every copy
// — as seen through all four read routes
void check_committed(KeystoneService& ks, const ObjectKey& key,
                     uint64_t checksum, size_t copies,
                     const std::vector<uint64_t>& digests) {
  CHECK(ks.object_exists(key));
  auto listed = ks.list_objects("");
  CHECK(listed.size() == 1 && listed[0].key == key &&
        listed[0].ncopies == copies);
  auto one = ks.get_workers(key);
  auto many = ks.batch_get_workers({key});
  CHECK(one.ok());
  CHECK(many.items.size() == 1 && many.items[0].status == 0);
  if (!one.ok() || many.items.size() != 1) return;
  for (const GetWorkersResponse* info : {&one.value(), &many.items[0].info}) {
    CHECK(info->checksum == checksum && info->size == kObj);
    CHECK(info->copies.size() == copies);
    for (const auto& c : info->copies) {
      CHECK(c.shards.size() == digests.size());
      for (size_t s = 0; s < c.shards.size() && s < digests.size(); ++s)
        CHECK(c.shards[s].digest == digests[s]);
    }
  }
}

void commit_table() {
  const ObjectKey key = "k";
  for (uint32_t repl = 1; repl <= 2; ++repl)
    for (int r = 0; r < kCommitRoutes; ++r) {
      auto ks = table_keystone();
      PlacementConfig pc;
      pc.replication = repl;
      CHECK(ks->put_start(key, kObj, pc).ok());
      const auto route = static_cast<CommitRoute>(r);
      uint64_t token = 0;
      if (route == TOKEN) {
        token = ks->create_put_session({{key, kObj, pc}});
        CHECK(token != 0);
        CHECK(ks->upsert_start_token(token).ok());
        CHECK(ks->commit_token(token, {1, 2}).code() ==
              ErrorCode::INVALID_ARGUMENT);  // one digest per object
        CHECK(ks->commit_token(token, {0xC0FFEE}).ok());
      } else {
        CHECK(complete_via(*ks, route, key, 0xC0FFEE) == 0);
      }
      check_committed(*ks, key, 0xC0FFEE, repl, {0xC0FFEE});
      if (route == TOKEN) {
        // the session survives a plain commit; release=true ends it
        CHECK(ks->upsert_start_token(token).ok());
        CHECK(ks->commit_token(token, {0xBEEF}, true).ok());
        check_committed(*ks, key, 0xBEEF, repl, {0xBEEF});
        CHECK(ks->upsert_start_token(token).code() == ErrorCode::SESSION_STALE);
        CHECK(ks->commit_token(token, {0xBEEF}).code() ==
              ErrorCode::SESSION_STALE);
        CHECK(ks->token_commits() == 2);
      } else {
        // a retried commit: same checksum succeeds, another one does not
        CHECK(complete_via(*ks, route, key, 0xC0FFEE) == 0);
        CHECK(complete_via(*ks, route, key, 0xBAD) ==
              code_of(ErrorCode::INVALID_STATE));
        check_committed(*ks, key, 0xC0FFEE, repl, {0xC0FFEE});
        CHECK(complete_via(*ks, route, "missing", 1) ==
              code_of(ErrorCode::OBJECT_NOT_FOUND));
      }
      ks->stop();
      std::printf("  commit    repl=%u %-18s committed, digest on %u copies\n",
                  repl, kCommitName[r], repl);
    }
  // a two-shard striped copy: per-shard digests need the right shape
  for (int r = 0; r < TOKEN; ++r)
    for (int wrong_shape = 0; wrong_shape < 2; ++wrong_shape) {
      auto ks = table_keystone();
      PlacementConfig pc;
      pc.max_workers_per_copy = 2;
      auto placed = ks->put_start(key, kObj, pc);
      CHECK(placed.ok() && placed.value().copies.size() == 1 &&
            placed.value().copies[0].shards.size() == 2);
      CHECK(ks->create_put_session({{key, kObj, pc}}) == 0);  // single-shard only
      std::vector<std::vector<uint64_t>> sd = {{11, 22}};
      if (wrong_shape) sd = {{11}};
      CHECK(complete_via(*ks, static_cast<CommitRoute>(r), key, 0xC0FFEE, sd) == 0);
      check_committed(*ks, key, 0xC0FFEE, 1,
                      wrong_shape ? std::vector<uint64_t>{0, 0}
                                  : std::vector<uint64_t>{11, 22});
      ks->stop();
      std::printf("  commit    striped %-18s %s\n", kCommitName[r],
                  wrong_shape ? "wrong shape: digests untouched"
                              : "digests recorded per shard");
    }
}

void read_table() {
  struct Row {
    const char* name;
    bool visible;
    ErrorCode get;
  };
  const Row rows[] = {{"absent", false, ErrorCode::OBJECT_NOT_FOUND},
                      {"pending", false, ErrorCode::OBJECT_NOT_COMMITTED},
                      {"committed", true, ErrorCode::OK},
                      {"expired", false, ErrorCode::OBJECT_EXPIRED}};
  for (int state = 0; state < 4; ++state)
    for (int batch_get = 0; batch_get < 2; ++batch_get) {
      auto ks = table_keystone();
      const ObjectKey key = "k";
      PlacementConfig pc;
      if (state == 3) pc.ttl_ms = 5;
      if (state >= 1) CHECK(ks->put_start(key, kObj, pc).ok());
      if (state >= 2) CHECK(ks->put_complete(key, 7).ok());
      if (state == 3)
        std::this_thread::sleep_for(std::chrono::milliseconds(12));
      auto get = [&] {
        if (!batch_get) return code_of(ks->get_workers(key).code());
        auto resp = ks->batch_get_workers({key});
        CHECK(resp.items.size() == 1);
        return resp.items.empty() ? -1 : resp.items[0].status;
      };
      const Row& row = rows[state];
      const bool exists = ks->object_exists(key);
      const size_t listed = ks->list_objects("").size();
      CHECK(exists == row.visible);
      CHECK(ks->batch_object_exists({key}) == std::vector<uint8_t>{exists});
      CHECK(listed == (row.visible ? 1u : 0u));
      const int32_t first = get();
      CHECK(first == code_of(row.get));
      if (state == 3) {
        // either get route removes the expired object on the way out
        CHECK(ks->get_cluster_stats().total_used == 0);
        CHECK(get() == code_of(ErrorCode::OBJECT_NOT_FOUND));
      } else {
        CHECK(get() == first);
        CHECK(ks->get_cluster_stats().total_used == (state ? kObj : 0));
      }
      ks->stop();
      std::printf("  read      %-9s %-17s exists=%d listed=%zu get=%d\n",
                  row.name, batch_get ? "batch_get_workers" : "get_workers",
                  exists, listed, first);
    }
}

void keystone_transitions() {
  admission_table();
  commit_table();
  read_table();
}

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

// The pool resolver under its callers' concurrency: views of two RAM_CPU
// pools taken by registry entry and by shm name through one shared mapper,
// each thread copying through view.base in a 4 KiB range of its own, while
// the registry gains and loses an unrelated entry.
void pool_view_storm() {
  constexpr uint64_t kPool = 1 << 20, kRange = 4096;
  constexpr int kThreads = 6;
  const PoolId ids[2] = {"storm_a", "storm_b"};
  std::unique_ptr<StorageBackend> pools[2];
  for (int p = 0; p < 2; ++p) {
    PoolConfig pc;
    pc.pool_id = ids[p];
    pc.storage_class = StorageClass::RAM_CPU;
    pc.size_bytes = kPool;
    auto b = create_storage_backend(pc, "selftest" + std::to_string(getpid()));
    CHECK(b.ok() && b.value()->initialize().ok());
    if (failures) return;
    pools[p] = std::move(b.value());
    LocalPools::inst().add(ids[p], pools[p]->base_ptr(), kPool, false, -1,
                           pools[p].get());
  }
  PoolMapper mapper;
  std::atomic<bool> stop{false};
  std::thread churn([&] {
    static uint8_t unrelated[64];
    while (!stop.load()) {
      LocalPools::inst().add("storm_tmp", unrelated, sizeof(unrelated), false, -1);
      CHECK(PoolMapper::local("storm_tmp").base == unrelated);
      LocalPools::inst().remove("storm_tmp");
    }
  });
  std::vector<std::thread> ts;
  for (int t = 0; t < kThreads; ++t)
    ts.emplace_back([&, t] {
      std::vector<uint8_t> out(kRange), in(kRange);
      for (int i = 0; i < 400; ++i) {
        const int p = i & 1;
        PoolView v = (t & 1) ? mapper.remote(pools[p]->access_info())
                             : PoolMapper::local(ids[p]);
        CHECK(v.base && !v.device && v.size == kPool);
        CHECK((v.local == pools[p].get()) == !(t & 1));
        const uint64_t off = t * kRange;
        CHECK(v.contains(off, kRange) && !v.contains(kPool - kRange, 2 * kRange));
        if (!v.base) return;
        std::fill(out.begin(), out.end(), static_cast<uint8_t>(t * 31 + i));
        std::memcpy(v.base + off, out.data(), kRange);
        std::memcpy(in.data(), v.base + off, kRange);
        CHECK(in == out);
      }
    });
  for (auto& t : ts) t.join();
  stop = true;
  churn.join();
  CHECK(!PoolMapper::local("storm_tmp").base);
  for (int p = 0; p < 2; ++p) {
    // what a thread wrote through either mapping, the backend reads
    std::vector<uint8_t> got(kRange);
    CHECK(pools[p]->read((kThreads - 1) * kRange, got.data(), kRange).ok());
    CHECK(got[0] == static_cast<uint8_t>((kThreads - 1) * 31 + 398 + p));
    LocalPools::inst().remove(ids[p]);
    CHECK(!PoolMapper::local(ids[p]).base);
  }
}

}  // namespace

int main() {
  std::setvbuf(stdout, nullptr, _IOLBF, 0);  // table rows stay whole in a log
  std::printf("pool_allocator_storm...\n");
  pool_allocator_storm();
  std::printf("range_allocator_storm...\n");
  range_allocator_storm();
  std::printf("coord_storm...\n");
  coord_storm();
  std::printf("keystone_storm...\n");
  keystone_storm();
  std::printf("keystone_transitions...\n");
  keystone_transitions();
  std::printf("v2_replace_storm...\n");
  v2_replace_storm();
  std::printf("coord_repl_storm...\n");
  coord_repl_storm();
  std::printf("placement_cache_storm...\n");
  placement_cache_storm();
  std::printf("fan_out_storm...\n");
  fan_out_storm();
  std::printf("pool_view_storm...\n");
  pool_view_storm();
  if (failures) {
    std::printf("SELFTEST FAILED (%d checks)\n", failures);
    return 1;
  }
  std::printf("SELFTEST OK\n");
  return 0;
}
