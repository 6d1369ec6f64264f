#include "blackbird/client/gpu_client.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <future>
#include <map>
#include <span>

#include <hip/hip_runtime_api.h>

#include "blackbird/client/batch_util.h"
#include "blackbird/client/batch_wire.h"
#include "blackbird/client/pool_mapper.h"
#include "blackbird/common/trace.h"
#include "blackbird/common/log.h"
#include "blackbird/gpu/hip_check.h"
#include "blackbird/rpc/methods.h"
#include "blackbird/worker/storage_backend.h"

namespace blackbird {

namespace M = rpc::methods;

namespace {
struct KeyMsg {
  std::string key;
  BB_FIELDS(key)
};
struct KeysMsg {
  std::vector<std::string> keys;
  BB_FIELDS(keys)
};

bool aligned16(const void* a, const void* b = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) &
          15) == 0;
}

// key_of(x) of every x in `range`, for the placement cache
template <typename Range, typename KeyOf>
PlacementCache::KeyList key_list(const Range& range, KeyOf key_of) {
  PlacementCache::KeyList list;
  list.reserve(std::size(range));
  for (const auto& x : range) list.push_back(&key_of(x));
  return list;
}

// a one-item batch's answer as the single call's
Result<void> first_status(const Result<std::vector<int32_t>>& r,
                          const ObjectKey& key) {
  if (!r.ok()) return r.error();
  if (r.value()[0] != 0)
    return Error{static_cast<ErrorCode>(r.value()[0]), key};
  return {};
}

bool any_striped(const std::vector<CopyPlacement>& copies) {
  for (const auto& c : copies)
    if (c.shards.size() > 1) return true;
  return false;
}

using StripeRange = GpuClient::StripeRange;
using ShardDigests = std::vector<std::vector<uint64_t>>;

// where item i's segments end in a list of nsegs
size_t seg_end(const std::vector<StripeRange>& ranges, size_t i, size_t nsegs) {
  return i + 1 < ranges.size() ? ranges[i + 1].first_seg : nsegs;
}

// every copy's object digest equals copy 0's
bool copies_agree(const std::vector<uint64_t>& obj_digests,
                  const StripeRange& r) {
  for (uint32_t c = 1; c < r.ncopies; ++c)
    if (obj_digests[r.first_obj + c] != obj_digests[r.first_obj]) return false;
  return true;
}

// An item's flat segment digests regrouped per copy, for the wire. Either
// from the copies themselves: copy c owns the next copies[c].shards.size()
// digests from r.first_seg on…
ShardDigests shard_digests_of(const StripeRange& r,
                              const std::vector<CopyPlacement>& copies,
                              const std::vector<uint64_t>& seg_digests) {
  ShardDigests out;
  out.reserve(copies.size());
  auto at = seg_digests.begin() + r.first_seg;
  for (const auto& c : copies) {
    out.emplace_back(at, at + c.shards.size());
    at += c.shards.size();
  }
  return out;
}
// …or from each kernel object's shard count (a patch session's lists)…
ShardDigests shard_digests_of(const StripeRange& r,
                              const std::vector<uint32_t>& copy_shards,
                              const std::vector<uint64_t>& shard_digests) {
  ShardDigests out;
  out.reserve(r.ncopies);
  auto at = shard_digests.begin() + r.first_seg;
  for (uint32_t c = 0; c < r.ncopies; ++c) {
    out.emplace_back(at, at + copy_shards[r.first_obj + c]);
    at += copy_shards[r.first_obj + c];
  }
  return out;
}
// …or from the launch's segment list: segs[k] of [r.first_seg, end) belongs
// to copy segs[k].obj - r.first_obj.
ShardDigests shard_digests_of(const StripeRange& r,
                              const std::vector<gpu::StripeSeg>& segs,
                              size_t end,
                              const std::vector<uint64_t>& seg_digests) {
  ShardDigests out(r.ncopies);
  for (size_t k = r.first_seg; k < end; ++k)
    out[segs[k].obj - r.first_obj].push_back(seg_digests[k]);
  return out;
}
}  // namespace

GpuClient::GpuClient(Client& base, int device) : c_(base), device_(device) {}

GpuClient::~GpuClient() {
  {
    // drain in-flight async batches before tearing streams down
    std::lock_guard<std::mutex> g(async_mu_);
    for (auto& [t, f] : async_)
      if (f.valid()) f.wait();
    async_.clear();
  }
  if (initialized_) {
    (void)hipSetDevice(device_);
    for (auto& s : streams_)
      if (s) (void)hipStreamDestroy(s);
    for (auto& s : fan_streams_)
      if (s) (void)hipStreamDestroy(s);
    if (staging_) (void)hipHostFree(staging_);
    for (void* p : staging_pool_) (void)hipHostFree(p);
  }
}

void* GpuClient::acquire_staging_buf() {
  {
    std::lock_guard<std::mutex> g(staging_pool_mu_);
    if (!staging_pool_.empty()) {
      void* p = staging_pool_.back();
      staging_pool_.pop_back();
      return p;
    }
  }
  void* p = nullptr;
  if (hipHostMalloc(&p, kFanBuf, hipHostMallocDefault) != hipSuccess)
    return nullptr;
  return p;
}

void GpuClient::release_staging_buf(void* p) {
  if (!p) return;
  std::lock_guard<std::mutex> g(staging_pool_mu_);
  staging_pool_.push_back(p);
}

Result<void> GpuClient::init() {
  if (initialized_) return {};
  if (!gpu::available()) return Error{ErrorCode::NO_GPU, "no MI355X visible"};
  BB_HIP_TRY(hipSetDevice(device_));
  for (auto& s : streams_)
    BB_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  for (auto& s : fan_streams_)
    BB_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  BB_HIP_TRY(hipHostMalloc(&staging_, staging_size_, hipHostMallocDefault));
  initialized_ = true;
  return {};
}

// Device-visible base of a pool — HBM local, IPC peer, or GPU-mapped host
// tier — or nullptr (staged path). `hint` is access info the caller already
// holds (a v1 shard carries it): with an endpoint in it no pool_access RPC
// is issued.
uint8_t* GpuClient::resolve_pool_base(const PoolId& pool_id, AccessInfo* access,
                                      const AccessInfo* hint) {
  PoolView v = PoolMapper::local(pool_id);
  if (!v.base) {
    // a pool of another process (one rank per GPU): IPC import or shm map.
    // An unmapped tier of this process comes this way too, for its endpoint.
    AccessInfo a;
    if (hint && !hint->endpoint.empty()) {
      a = *hint;
    } else {
      auto r = c_.pool_access(pool_id);
      if (!r.ok()) return nullptr;
      a = std::move(r.value());
    }
    v = c_.mapper_->remote(a);
    if (access) *access = std::move(a);
  }
  if (!v.base || v.device) return v.base;
  // host pool (pinned/shm tier), local or shm-mapped: pin+map once so the
  // GPU addresses it directly (PCIe DMA) instead of staging through a bounce
  return static_cast<uint8_t*>(
      c_.mapper_->host_dev_map(pool_id, v.base, v.size));
}

uint8_t* GpuClient::resolve_device_ptr(const ShardPlacement& s) {
  uint8_t* base = resolve_pool_base(s.pool_id, nullptr, &s.access);
  return base ? base + s.offset : nullptr;
}

// The pool table of a v2 response: `base` is the device-visible base of each
// pool, nullptr sending its ranges through staging.
std::vector<PoolRef> GpuClient::resolve_pools(const std::vector<PoolId>& ids) {
  return resolve_pool_table(ids, [this](const PoolId& id, AccessInfo* a) {
    return resolve_pool_base(id, a);
  });
}

// Routes the (user buffer ↔ pool range) transfers of one batch: a
// device-visible range joins the fused copy list (one kernel launch at
// flush()) or, with fused copies off, goes out as hipMemcpyAsync on the
// rotating streams; a range that is not device-visible is staged through
// pinned host memory — queued for the caller's fan-out (v2 batches), or done
// on the spot (v1 paths, whose shards are few and large).
template <bool Put>
struct GpuClient::Router {
  using User = std::conditional_t<Put, const uint8_t*, uint8_t*>;
  using StagedPtr = std::conditional_t<Put, const void*, void*>;

  GpuClient& g;
  const bool fused;
  const bool defer_staged;
  std::vector<gpu::CopyDesc> copies;  // fused copy list
  int si = 0;                         // SDMA copies issued (stream rotation)
  std::vector<std::pair<ShardPlacement, StagedPtr>> staged;
  std::vector<uint32_t> staged_idx;   // item of staged[k]
  // items that bypass add(): they ride the copy+digest kernel instead
  std::vector<gpu::PutDesc> hashed;
  std::vector<uint32_t> hashed_idx;
  std::vector<uint32_t> plain_idx;    // items moved by add() alone
  std::vector<uint64_t> hashed_digests, plain_digests;  // launch_put() output

  Router(GpuClient& gc, bool fused_copy, bool defer)
      : g(gc), fused(fused_copy), defer_staged(defer) {}

  // v1: one shard, already resolved (pool_ptr nullptr = not device-visible)
  Result<void> add(User user, uint8_t* pool_ptr, const ShardPlacement& s,
                   uint32_t item) {
    if (pool_ptr) return direct(user, pool_ptr, s.length);
    return stage(s, user, item);
  }
  // v1: every shard of one copy, back to back in the user buffer
  Result<void> add_copy(User user, const CopyPlacement& copy, uint32_t item) {
    for (const auto& s : copy.shards) {
      BB_RETURN_IF_ERROR(add(user, g.resolve_device_ptr(s), s, item));
      user += s.length;
    }
    return {};
  }
  // v2: a range of a pool-table entry
  Result<void> add(User user, const PoolRef& pr, uint64_t offset,
                   uint64_t nbytes, uint32_t item) {
    if (pr.base) return direct(user, pr.base + offset, nbytes);
    return stage(pr.shard(offset, nbytes), user, item);
  }

  // launch the fused copy list on streams_[0]
  Result<void> flush() {
    if (copies.empty()) return {};
    return gpu::batched_copy(copies.data(),
                             static_cast<uint32_t>(copies.size()),
                             g.streams_[0]);
  }
  // the copy+digest list on streams_[2] (synchronizes that stream itself)
  Result<std::vector<uint64_t>> run_hashed() {
    std::vector<uint64_t> digests(hashed.size(), 0);
    BB_RETURN_IF_ERROR(gpu::fused_put(hashed.data(),
                                      static_cast<uint32_t>(hashed.size()),
                                      digests.data(), g.streams_[2],
                                      g.warm_tail(Put)));
    return digests;
  }
  // Everything a put batch launches, in order: the copy list (stream 0), one
  // digest launch over the SOURCE buffers of the plain items (stream 1, so
  // it overlaps the SDMA copies), the copy+digest list (stream 2); then the
  // sync. Fills plain_digests / hashed_digests.
  Result<void> launch_put(const std::vector<DevPutItem>& items, bool checksum) {
    BB_RETURN_IF_ERROR(flush());
    plain_digests.assign(plain_idx.size(), 0);
    if (checksum) {
      auto r = g.digest_items(
          plain_idx, [&](uint32_t i) { return items[i].ptr; },
          [&](uint32_t i) { return items[i].size; }, g.streams_[1]);
      if (!r.ok()) return r.error();
      plain_digests = std::move(r.value());
    }
    auto r = run_hashed();
    if (!r.ok()) return r.error();
    hashed_digests = std::move(r.value());
    return sync();
  }
  // Everything a get batch launches after routing: the copy list (stream
  // 0), the copy+digest list (stream 2; verifies as it gathers), the sync,
  // then with `verify` one digest launch over what the plain items fetched
  // (stream 0). meta_of(i) → {size, recorded checksum (0 = none)} of item i.
  template <typename MetaOf>
  Result<void> finish_get(const std::vector<DevGetItem>& items, bool verify,
                          MetaOf meta_of, std::vector<int32_t>& statuses) {
    auto check = [&](const std::vector<uint32_t>& idx,
                     const std::vector<uint64_t>& got, bool zero_passes) {
      for (size_t j = 0; j < idx.size(); ++j) {
        const uint64_t want = meta_of(idx[j]).second;
        if (got[j] != want && !(zero_passes && want == 0))
          statuses[idx[j]] = static_cast<int32_t>(ErrorCode::CHECKSUM_MISMATCH);
      }
    };
    BB_RETURN_IF_ERROR(flush());
    auto hashed_got = run_hashed();
    if (!hashed_got.ok()) return hashed_got.error();
    check(hashed_idx, hashed_got.value(), false);
    BB_RETURN_IF_ERROR(sync());
    if (!verify) return {};
    auto got = g.digest_items(
        plain_idx, [&](uint32_t i) { return items[i].ptr; },
        [&](uint32_t i) { return meta_of(i).first; }, g.streams_[0]);
    if (!got.ok()) return got.error();
    check(plain_idx, got.value(), true);
    return {};
  }
  // only streams that carried work: stream 0 (fused list) and the first
  // `si` rotating SDMA streams (checksum_batch and fused_put synchronize
  // their own streams internally)
  Result<void> sync() {
    if (!copies.empty()) BB_HIP_TRY(hipStreamSynchronize(g.streams_[0]));
    for (int j = 0; j < std::min(si, kStreams); ++j)
      BB_HIP_TRY(hipStreamSynchronize(g.streams_[j]));
    return {};
  }

 private:
  Result<void> direct(User user, uint8_t* pool_ptr, uint64_t nbytes) {
    const void* src = Put ? static_cast<const void*>(user) : pool_ptr;
    void* dst = Put ? static_cast<void*>(pool_ptr)
                    : const_cast<uint8_t*>(user);
    if (fused) {
      copies.push_back({src, dst, nbytes});
      return {};
    }
    BB_HIP_TRY(hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToDevice,
                              g.streams_[si % kStreams]));
    ++si;
    return {};
  }
  template <typename Shard>
  Result<void> stage(Shard&& s, User user, uint32_t item) {
    if (defer_staged) {
      staged.emplace_back(std::forward<Shard>(s), user);
      staged_idx.push_back(item);
      return {};
    }
    if constexpr (Put) return g.staged_write(s, user);
    else return g.staged_read(s, user);
  }
};

// The striped items of one v1 batch that ride ONE gpu::fused_stripe launch:
// every shard is a segment, every copy one kernel "object" — the launch
// moves the bytes and yields each shard's digest and each copy's object
// digest from a single read. A copy joins only when the planner accepts its
// shard lengths and every shard resolves to a 16B-aligned device pointer;
// the caller routes everything else the general way.
struct GpuClient::StripeBatch {
  using Entry = StripeRange;
  template <bool Put>
  using User = std::conditional_t<Put, const uint8_t*, uint8_t*>;
  std::vector<gpu::StripeSeg> segs;
  std::vector<uint64_t> obj_sizes;
  std::vector<Entry> entries;
  std::vector<uint64_t> seg_digests, obj_digests;  // run() output

  // All of `copy` as one new kernel object, `user` holding the object's
  // bytes back to back (Put: the source; get: the destination). false =
  // not fusable, nothing added.
  template <bool Put>
  bool add_copy(GpuClient& g, User<Put> user, uint64_t size,
                const CopyPlacement& copy) {
    return add_shards<Put>(
        user, size, copy.shards.size(),
        [&](size_t k) { return copy.shards[k].length; },
        [&](size_t k) { return g.resolve_device_ptr(copy.shards[k]); });
  }
  // The same from a striped placement-cache entry (copy 0 as recorded).
  template <bool Put>
  bool add_cached(GpuClient& g, User<Put> user,
                  const PlacementCache::Entry& e) {
    return add_shards<Put>(
        user, e.size, e.shards.size(),
        [&](size_t k) { return e.shards[k].length; },
        [&](size_t k) -> uint8_t* {
          uint8_t* base = g.resolve_pool_base(e.shards[k].pool_id);
          return base ? base + e.shards[k].offset : nullptr;
        });
  }
  template <bool Put, typename LenOf, typename PtrOf>
  bool add_shards(User<Put> user, uint64_t size, size_t nshards, LenOf len_of,
                  PtrOf ptr_of) {
    std::vector<uint64_t> lens;
    lens.reserve(nshards);
    for (size_t k = 0; k < nshards; ++k) lens.push_back(len_of(k));
    const auto plan = gpu::plan_stripe(size, lens);
    if (!plan) return false;
    const size_t mark = segs.size();
    const uint32_t obj = static_cast<uint32_t>(obj_sizes.size());
    for (size_t k = 0; k < plan->size(); ++k) {
      uint8_t* pool_ptr = ptr_of(k);
      if (!pool_ptr || !aligned16(pool_ptr, user + (*plan)[k].offset)) {
        segs.resize(mark);
        return false;
      }
      auto* slice = const_cast<uint8_t*>(user) + (*plan)[k].offset;
      if constexpr (Put)
        segs.push_back({slice, pool_ptr, (*plan)[k].nbytes, (*plan)[k].first_tile, obj});
      else
        segs.push_back({pool_ptr, slice, (*plan)[k].nbytes, (*plan)[k].first_tile, obj});
    }
    obj_sizes.push_back(size);
    return true;
  }
  // drop everything added since the marks (an item whose later copy failed)
  void rewind(size_t seg_mark, size_t obj_mark) {
    segs.resize(seg_mark);
    obj_sizes.resize(obj_mark);
  }
  // the launch (synchronizes `stream` itself); no launch for an empty batch
  Result<void> run(hipStream_t stream) {
    seg_digests.assign(segs.size(), 0);
    obj_digests.assign(obj_sizes.size(), 0);
    return gpu::fused_stripe(segs.data(), static_cast<uint32_t>(segs.size()),
                             obj_sizes.data(),
                             static_cast<uint32_t>(obj_sizes.size()),
                             seg_digests.data(), obj_digests.data(), stream);
  }
};

// One batched digest launch over items[indices]: out[j] is the digest of
// ptr_of(indices[j]) .. + size_of(indices[j]). No launch for an empty list.
template <typename PtrOf, typename SizeOf>
Result<std::vector<uint64_t>> GpuClient::digest_items(
    const std::vector<uint32_t>& indices, PtrOf ptr_of, SizeOf size_of,
    hipStream_t stream) {
  std::vector<uint64_t> out(indices.size(), 0);
  if (indices.empty()) return out;
  std::vector<const void*> ptrs;
  std::vector<uint64_t> sizes;
  ptrs.reserve(indices.size());
  sizes.reserve(indices.size());
  for (auto i : indices) {
    ptrs.push_back(ptr_of(i));
    sizes.push_back(size_of(i));
  }
  BB_RETURN_IF_ERROR(gpu::checksum_batch(ptrs.data(), sizes.data(),
                                         static_cast<uint32_t>(ptrs.size()),
                                         out.data(), device_, stream));
  return out;
}

// BATCH_PUT_COMPLETE for what a put batch transferred: the plain group
// (skipping items a failed staged write marked) and the copy+digest group,
// whose digests sit `stride` apart (one per replica). v1 attaches per-shard
// digests and applies the per-item answers; v2 does neither.
Result<void> GpuClient::complete_puts(
    const std::vector<DevPutItem>& items, const Router<true>& rt, size_t stride,
    std::map<uint32_t, std::vector<std::vector<uint64_t>>>* shard_digests,
    std::vector<int32_t>& statuses, bool apply_statuses) {
  std::vector<PutCompleteRequest> reqs;
  std::vector<uint32_t> order;
  for (size_t j = 0; j < rt.plain_idx.size(); ++j) {
    const uint32_t i = rt.plain_idx[j];
    if (statuses[i] != 0) continue;
    PutCompleteRequest pc{items[i].key, rt.plain_digests[j], {}};
    if (shard_digests)
      if (auto it = shard_digests->find(i); it != shard_digests->end())
        pc.shard_digests = std::move(it->second);
    reqs.push_back(std::move(pc));
    order.push_back(i);
  }
  for (size_t j = 0; j < rt.hashed_idx.size(); ++j) {
    reqs.push_back(PutCompleteRequest{items[rt.hashed_idx[j]].key,
                                      rt.hashed_digests[j * stride], {}});
    order.push_back(rt.hashed_idx[j]);
  }
  return c_.complete_by_keys(reqs, order, apply_statuses ? &statuses : nullptr);
}

// BATCH_PUT_CANCEL for the items whose transfer failed
void GpuClient::cancel_failed(const std::vector<DevPutItem>& items,
                              const std::vector<int32_t>& statuses) {
  std::vector<ObjectKey> cancels;
  for (size_t i = 0; i < items.size(); ++i)
    if (statuses[i] == static_cast<int32_t>(ErrorCode::TRANSFER_FAILED))
      cancels.push_back(items[i].key);
  c_.cancel_puts(cancels);
}

Result<void> GpuClient::staged_write(const ShardPlacement& s, const void* dev_src) {
  // D2H into pinned staging, then the host path (SHM memcpy or TCP frame).
  std::lock_guard<std::mutex> g(staging_mu_);  // async batches share staging_
  return staged_write_buf(s, dev_src, staging_, staging_size_);
}

Result<void> GpuClient::staged_read_buf(const ShardPlacement& s, void* dev_dst,
                                        void* staging, uint64_t staging_size) {
  uint64_t done = 0;
  while (done < s.length) {
    uint64_t chunk = std::min(s.length - done, staging_size);
    ShardPlacement part = s;
    part.offset = s.offset + done;
    part.length = chunk;
    BB_RETURN_IF_ERROR(c_.read_shard(part, staging));
    BB_RETURN_IF_ERROR(gpu::copy_sync(
        static_cast<uint8_t*>(dev_dst) + done, staging, chunk,
        hipMemcpyHostToDevice));
    done += chunk;
  }
  return {};
}

Result<void> GpuClient::staged_write_buf(const ShardPlacement& s,
                                         const void* dev_src, void* staging,
                                         uint64_t staging_size) {
  uint64_t done = 0;
  while (done < s.length) {
    uint64_t chunk = std::min(s.length - done, staging_size);
    BB_RETURN_IF_ERROR(gpu::copy_sync(
        staging, static_cast<const uint8_t*>(dev_src) + done, chunk,
        hipMemcpyDeviceToHost));
    ShardPlacement part = s;
    part.offset = s.offset + done;
    part.length = chunk;
    BB_RETURN_IF_ERROR(c_.write_shard(part, staging));
    done += chunk;
  }
  return {};
}

Result<void> GpuClient::staged_write_many(
    const std::vector<std::pair<ShardPlacement, const void*>>& work) {
  if (work.empty()) return {};
  if (work.size() == 1) return staged_write(work[0].first, work[0].second);
  const uint64_t half = kFanBuf / 2;
  // items that fit a half-buffer ride a 1-deep D2H pipeline (the next
  // item's device→pinned copy flies while the current one is written to
  // the backend); oversized items take the chunked path
  std::vector<size_t> small, large;
  for (size_t i = 0; i < work.size(); ++i)
    (work[i].first.length <= half ? small : large).push_back(i);
  const int nthreads =
      std::min<int>(kFanThreads, static_cast<int>(work.size()));
  std::atomic<size_t> next{0};
  std::atomic<size_t> lnext{0};
  std::vector<std::future<Result<void>>> futs;
  for (int t = 0; t < nthreads; ++t)
    futs.push_back(std::async(std::launch::async, [&, t]() -> Result<void> {
      void* buf = acquire_staging_buf();
      if (!buf) return Error{ErrorCode::HIP_ERROR, "staging alloc"};
      uint8_t* halves[2] = {static_cast<uint8_t*>(buf),
                            static_cast<uint8_t*>(buf) + half};
      hipStream_t st = fan_streams_[t % kFanThreads];
      hipEvent_t ev[2] = {};
      Result<void> rc{};
      auto fail = [&](Result<void> r) { if (rc.ok()) rc = r; };
      for (auto& e : ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
          fail(Error{ErrorCode::HIP_ERROR, "event create"});
      if (rc.ok()) {
        size_t inflight = SIZE_MAX;  // index whose D2H is on halves[ib^1]
        int ib = 0;
        for (;;) {
          size_t k = next.fetch_add(1);
          const bool have_new = k < small.size();
          if (have_new) {
            auto& [sp, src] = work[small[k]];
            if (hipMemcpyAsync(halves[ib], src, sp.length,
                               hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipEventRecord(ev[ib], st) != hipSuccess) {
              fail(Error{ErrorCode::HIP_ERROR, "staged D2H"});
              break;
            }
          }
          if (inflight != SIZE_MAX) {
            // wait only for the PREVIOUS D2H (FIFO stream: its event fired
            // before the new copy completes), then write it out while the
            // new copy flies
            if (hipEventSynchronize(ev[ib ^ 1]) != hipSuccess) {
              fail(Error{ErrorCode::HIP_ERROR, "staged D2H sync"});
              break;
            }
            auto r = c_.write_shard(work[inflight].first, halves[ib ^ 1]);
            if (!r.ok()) {
              fail(r);
              break;
            }
          }
          if (!have_new) break;
          inflight = small[k];
          ib ^= 1;
        }
        // chunked path for oversized items
        for (size_t k = lnext.fetch_add(1); rc.ok() && k < large.size();
             k = lnext.fetch_add(1)) {
          auto r = staged_write_buf(work[large[k]].first, work[large[k]].second,
                                    buf, kFanBuf);
          if (!r.ok()) fail(r);
        }
      }
      for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
      release_staging_buf(buf);
      return rc;
    }));
  for (auto& f : futs) BB_RETURN_IF_ERROR(f.get());
  return {};
}

Result<void> GpuClient::staged_read(const ShardPlacement& s, void* dev_dst) {
  std::lock_guard<std::mutex> g(staging_mu_);  // async batches share staging_
  return staged_read_buf(s, dev_dst, staging_, staging_size_);
}

Result<void> GpuClient::staged_read_many(
    const std::vector<std::pair<ShardPlacement, void*>>& work) {
  if (work.empty()) return {};
  if (work.size() == 1) return staged_read(work[0].first, work[0].second);
  // one staging buffer per thread; a thread stops at its first error
  std::vector<Result<void>> rcs(kFanThreads);
  fan_out_threads(work.size(), kFanThreads, [&](int t, auto& next) {
    void* buf = acquire_staging_buf();
    if (!buf) {
      rcs[t] = Error{ErrorCode::HIP_ERROR, "staging alloc"};
      return;
    }
    for (size_t i; rcs[t].ok() && next(i);)
      rcs[t] = staged_read_buf(work[i].first, work[i].second, buf, kFanBuf);
    release_staging_buf(buf);
  });
  for (auto& r : rcs)
    if (!r.ok()) return r.error();
  return {};
}

// -------------------------------------------------------------- single ops

Result<void> GpuClient::put_device(const ObjectKey& key, const void* dev_ptr,
                                   uint64_t size, const PlacementConfig& cfg) {
  return first_status(batch_put_device({DevPutItem{key, dev_ptr, size}}, cfg),
                      key);
}

Result<uint64_t> GpuClient::get_device(const ObjectKey& key, void* dev_ptr,
                                       uint64_t capacity, bool verify) {
  // (the placement cache is deliberately NOT used here: for one object the
  // copy+digest kernel launch costs more than the metadata RPC it saves —
  // measured 38 µs vs 21 µs at 1 MiB. Batched gets ride the cache.)
  auto meta = c_.meta_call<KeyMsg, GetWorkersResponse>(M::GET_WORKERS,
                                                        KeyMsg{key});
  if (!meta.ok()) return meta.error();
  if (meta->size > capacity)
    return Error{ErrorCode::SIZE_MISMATCH, "device buffer too small"};
  BB_RETURN_IF_ERROR(init());
  BB_HIP_TRY(hipSetDevice(device_));

  Error last{ErrorCode::NO_PLACEMENT, "no copies"};
  for (const auto& copy : meta->copies) {
    // one object: always plain copies on the rotating streams (a kernel
    // launch costs more than it saves here), staged shards on the spot
    Router<false> rt(*this, /*fused_copy=*/false, /*defer=*/false);
    auto r = rt.add_copy(static_cast<uint8_t*>(dev_ptr), copy, 0);
    BB_RETURN_IF_ERROR(rt.sync());
    if (!r.ok()) {
      last = r.error();
      continue;
    }
    if (verify && meta->checksum != 0) {
      auto cs = gpu::checksum_sync(dev_ptr, meta->size, device_, streams_[0]);
      if (!cs.ok()) return cs.error();
      if (cs.value() != meta->checksum)
        return Error{ErrorCode::CHECKSUM_MISMATCH, key};
    }
    return meta->size;
  }
  return last;
}

// ----------------------------------------------------------- ranged access

Result<std::vector<int32_t>> GpuClient::batch_get_device_range(
    const std::vector<DevRangeGet>& items) {
  std::vector<int32_t> statuses(items.size(), 0);
  if (items.empty()) return statuses;
  BB_RETURN_IF_ERROR(init());
  BB_HIP_TRY(hipSetDevice(device_));
  KeysMsg req;
  for (const auto& it : items) req.keys.push_back(it.key);
  auto resp = c_.meta_call<KeysMsg, BatchGetWorkersResponse>(
      M::BATCH_GET_WORKERS, req, c_.opts_.rpc_timeout_ms);
  if (!resp.ok()) return resp.error();
  if (resp->items.size() != items.size())
    return Error{ErrorCode::PROTOCOL_ERROR, "batch_get_workers: item count"};

  std::vector<gpu::CopyDesc> descs;  // the one batched_copy launch
  for (size_t i = 0; i < items.size(); ++i) {
    const auto& it = items[i];
    const auto& info = resp->items[i].info;
    if (resp->items[i].status != 0) {
      statuses[i] = resp->items[i].status;
      continue;
    }
    if (!range_inside(it.offset, it.length, info.size)) {
      statuses[i] = static_cast<int32_t>(ErrorCode::INVALID_ARGUMENT);
      continue;
    }
    statuses[i] = static_cast<int32_t>(ErrorCode::NO_PLACEMENT);
    for (const auto& copy : info.copies) {
      auto pieces =
          gpu::range_pieces(info.size, shard_lens_of(copy), it.offset, it.length);
      if (!pieces) continue;  // the copy does not cover the object
      const size_t mark = descs.size();
      Result<void> r{};
      for (const auto& p : *pieces) {
        const ShardPlacement& s = copy.shards[p.shard];
        uint8_t* user = static_cast<uint8_t*>(it.ptr) + (p.obj_off - it.offset);
        if (uint8_t* pool = resolve_device_ptr(s)) {
          descs.push_back({pool + p.shard_off, user, p.nbytes});
          continue;
        }
        if (s.length <= staging_size_) {
          // the whole shard into staging (what every tier serves), then the
          // slice
          std::lock_guard<std::mutex> g(staging_mu_);
          r = c_.read_shard(s, staging_);
          if (r.ok())
            r = gpu::copy_sync(user, static_cast<uint8_t*>(staging_) + p.shard_off,
                               p.nbytes, hipMemcpyHostToDevice);
        } else {
          r = staged_read(sub_shard(s, p.shard_off, p.nbytes), user);
        }
        if (!r.ok()) break;
      }
      if (r.ok()) {
        statuses[i] = 0;
        break;
      }
      descs.resize(mark);  // next replica
      statuses[i] = static_cast<int32_t>(r.code());
    }
  }
  if (!descs.empty()) {
    BB_RETURN_IF_ERROR(gpu::batched_copy(
        descs.data(), static_cast<uint32_t>(descs.size()), streams_[0]));
    BB_HIP_TRY(hipStreamSynchronize(streams_[0]));
  }
  return statuses;
}

Result<void> GpuClient::get_device_range(const ObjectKey& key, uint64_t offset,
                                         void* dev_ptr, uint64_t length) {
  return first_status(
      batch_get_device_range({DevRangeGet{key, offset, dev_ptr, length}}), key);
}

Result<void> GpuClient::patch_by_rewrite(const DevRangePatch& item,
                                         const GetWorkersResponse& info) {
  if (!range_inside(item.offset, item.length, info.size))
    return Error{ErrorCode::INVALID_ARGUMENT, "range past the end of " + item.key};
  void* tmp = nullptr;
  BB_HIP_TRY(hipMalloc(&tmp, std::max<uint64_t>(info.size, 16)));
  auto run = [&]() -> Result<void> {
    auto got = get_device(item.key, tmp, info.size, /*verify=*/true);
    if (!got.ok()) return got.error();
    BB_RETURN_IF_ERROR(gpu::copy_sync(static_cast<uint8_t*>(tmp) + item.offset,
                                      item.ptr, item.length,
                                      hipMemcpyDeviceToDevice));
    PlacementConfig cfg;
    cfg.replace = true;
    cfg.replication = static_cast<uint32_t>(info.copies.size());
    for (const auto& c : info.copies)
      cfg.max_workers_per_copy = std::max<uint32_t>(
          cfg.max_workers_per_copy, static_cast<uint32_t>(c.shards.size()));
    if (!info.copies.empty() && !info.copies[0].shards.empty())
      cfg.preferred_class = info.copies[0].shards[0].storage_class;
    return put_device(item.key, tmp, info.size, cfg);
  };
  auto r = run();
  (void)hipFree(tmp);
  return r;
}

Result<std::vector<int32_t>> GpuClient::batch_patch_device(
    const std::vector<DevRangePatch>& items, BatchPatchSession* sess) {
  std::vector<int32_t> statuses(items.size(), 0);
  if (items.empty()) return statuses;
  BB_RETURN_IF_ERROR(init());
  BB_HIP_TRY(hipSetDevice(device_));
  if (auto fast = try_session_patch(items, sess)) return std::move(*fast);
  std::vector<ObjectKey> keys;
  for (const auto& it : items) keys.push_back(it.key);
  auto started = c_.patch_start(keys);
  if (!started.ok()) return started.error();
  // the patched keys leave the cache whatever becomes of them; this also
  // unbinds every session
  cache_.erase(key_list(
      keys, [](const ObjectKey& k) -> const ObjectKey& { return k; }));

  // the one fused_patch launch: every copy of an item is a kernel object of
  // its own, so diverged replicas show as different digests. An item's range
  // counts shards (the digest lists), not the patched pieces.
  std::vector<gpu::PatchSeg> segs;
  std::vector<gpu::PatchEdge> edges;  // patch_edge_tiles_: tiles patched in part
  std::vector<uint64_t> shard_lens, shard_old, obj_sizes, obj_old;
  std::vector<uint32_t> copy_shards;  // per kernel object; a session keeps it
  std::vector<StripeRange> fused;
  std::vector<uint32_t> rewrite;  // item indices
  std::vector<GetWorkersResponse> rewrite_info(items.size());
  std::vector<ObjectKey> aborts;

  for (size_t i = 0; i < items.size(); ++i) {
    const auto& it = items[i];
    auto& got = started->items[i];
    if (got.status == static_cast<int32_t>(ErrorCode::INVALID_STATE)) {
      // no recorded checksum, no state changed: what is there to rewrite?
      auto meta = c_.meta_call<KeyMsg, GetWorkersResponse>(
          M::GET_WORKERS, KeyMsg{it.key}, c_.opts_.rpc_timeout_ms);
      if (!meta.ok()) {
        statuses[i] = static_cast<int32_t>(meta.code());
        continue;
      }
      rewrite_info[i] = std::move(meta.value());
      rewrite.push_back(static_cast<uint32_t>(i));
      continue;
    }
    if (got.status != 0) {
      statuses[i] = got.status;
      continue;
    }
    const GetWorkersResponse& info = got.info;
    if (!range_inside(it.offset, it.length, info.size)) {
      statuses[i] = static_cast<int32_t>(ErrorCode::INVALID_ARGUMENT);
      aborts.push_back(it.key);
      continue;
    }
    const size_t seg_mark = segs.size(), edge_mark = edges.size(),
                 shard_mark = shard_lens.size(), obj_mark = obj_sizes.size();
    bool in_place = !info.copies.empty();
    for (size_t c = 0; in_place && c < info.copies.size(); ++c) {
      const auto& copy = info.copies[c];
      // whole-tile runs, and with patch_edge_tiles_ the edge tiles around them
      std::optional<std::vector<gpu::RangePiece>> pieces;
      std::vector<gpu::EdgePiece> edge_pieces;
      if (patch_edge_tiles_) {
        if (auto plan = gpu::plan_patch_bytes(info.size, shard_lens_of(copy),
                                              it.offset, it.length)) {
          pieces = std::move(plan->runs);
          edge_pieces = std::move(plan->edges);
        }
      } else {
        pieces = gpu::plan_patch(info.size, shard_lens_of(copy), it.offset,
                                 it.length);
      }
      if (!pieces) {
        in_place = false;
        break;
      }
      const uint32_t shard0 = static_cast<uint32_t>(shard_lens.size());
      const uint32_t obj = static_cast<uint32_t>(obj_sizes.size());
      for (const auto& s : copy.shards) {
        if (s.digest == 0) in_place = false;
        shard_lens.push_back(s.length);
        shard_old.push_back(s.digest);
      }
      obj_sizes.push_back(info.size);
      obj_old.push_back(info.checksum);
      copy_shards.push_back(static_cast<uint32_t>(copy.shards.size()));
      for (const auto& p : *pieces) {
        uint8_t* pool = resolve_device_ptr(copy.shards[p.shard]);
        const uint8_t* src =
            static_cast<const uint8_t*>(it.ptr) + (p.obj_off - it.offset);
        if (!pool || !aligned16(pool + p.shard_off, src)) {
          in_place = false;
          break;
        }
        segs.push_back({src, pool + p.shard_off, p.nbytes,
                        p.shard_off / digest::kTileBytes,
                        p.obj_off / digest::kTileBytes, shard0 + p.shard, obj});
      }
      // edges go byte by byte: any device-visible address will do
      for (size_t k = 0; in_place && k < edge_pieces.size(); ++k) {
        const auto& e = edge_pieces[k];
        uint8_t* pool = resolve_device_ptr(copy.shards[e.shard]);
        if (!pool) {
          in_place = false;
          break;
        }
        edges.push_back({static_cast<const uint8_t*>(it.ptr) + e.src_off,
                         pool + e.shard_tile * digest::kTileBytes, e.lo, e.hi,
                         e.valid, e.shard_tile, e.obj_tile, shard0 + e.shard,
                         obj});
      }
    }
    if (!in_place) {
      segs.resize(seg_mark);
      edges.resize(edge_mark);
      shard_lens.resize(shard_mark);
      shard_old.resize(shard_mark);
      obj_sizes.resize(obj_mark);
      obj_old.resize(obj_mark);
      copy_shards.resize(obj_mark);
      aborts.push_back(it.key);
      rewrite_info[i] = info;
      rewrite.push_back(static_cast<uint32_t>(i));
      continue;
    }
    fused.push_back({static_cast<uint32_t>(i), static_cast<uint32_t>(obj_mark),
                     static_cast<uint32_t>(info.copies.size()),
                     static_cast<uint32_t>(shard_mark)});
  }
  c_.patch_abort(aborts);

  if (!fused.empty()) {
    std::vector<uint64_t> shard_new(shard_lens.size()), obj_new(obj_sizes.size());
    auto launched = gpu::fused_patch(
        segs.data(), static_cast<uint32_t>(segs.size()), shard_lens.data(),
        shard_old.data(), static_cast<uint32_t>(shard_lens.size()),
        obj_sizes.data(), obj_old.data(), static_cast<uint32_t>(obj_sizes.size()),
        shard_new.data(), obj_new.data(), streams_[2], edges.data(),
        static_cast<uint32_t>(edges.size()));
    std::vector<ObjectKey> cancels;
    std::vector<PutCompleteRequest> reqs;
    std::vector<uint32_t> order;
    for (const auto& f : fused) {
      const ObjectKey& key = items[f.item].key;
      if (!launched.ok()) {  // torn
        statuses[f.item] = static_cast<int32_t>(launched.code());
        cancels.push_back(key);
        continue;
      }
      if (!copies_agree(obj_new, f)) {
        statuses[f.item] = static_cast<int32_t>(ErrorCode::CHECKSUM_MISMATCH);
        cancels.push_back(key);
        continue;
      }
      reqs.push_back(PutCompleteRequest{
          key, obj_new[f.first_obj],
          shard_digests_of(f, started->items[f.item].info.copies, shard_new)});
      order.push_back(f.item);
    }
    c_.cancel_puts(cancels);
    // a session for the steps to come: the whole batch rode this launch and
    // will commit. Opened before the commit, while PENDING pins the
    // placements the run list points into.
    if (sess) {
      sess->end();
      if (fused.size() == items.size() && reqs.size() == items.size()) {
        std::vector<std::pair<ObjectKey, uint64_t>> objects;
        objects.reserve(items.size());
        for (const auto& f : fused)
          objects.emplace_back(items[f.item].key, obj_sizes[f.first_obj]);
        if (auto t = c_.open_session(objects, /*allow_striped=*/true);
            t.ok() && t.value() != 0) {
          sess->token = t.value();
          sess->bound = items;
          sess->segs = std::move(segs);
          sess->edges = std::move(edges);
          sess->shard_lens = std::move(shard_lens);
          sess->obj_sizes = std::move(obj_sizes);
          sess->copy_shards = std::move(copy_shards);
          sess->ranges = std::move(fused);
        }
      }
    }
    if (!reqs.empty()) {
      BB_RETURN_IF_ERROR(c_.complete_by_keys(reqs, order, &statuses));
      for (uint32_t i : order)
        if (statuses[i] == 0) ++patched_fused_items_;
      // the first step commits by key: an item that did not leaves no session
      if (sess)
        for (uint32_t i : order)
          if (statuses[i] != 0) sess->end();
    }
  } else if (sess) {
    sess->end();
  }

  for (uint32_t i : rewrite) {
    auto r = patch_by_rewrite(items[i], rewrite_info[i]);
    statuses[i] = static_cast<int32_t>(r.code());
    if (r.ok()) ++patched_rewrite_items_;
  }
  return statuses;
}

Result<void> GpuClient::patch_device(const ObjectKey& key, uint64_t offset,
                                     const void* dev_ptr, uint64_t length) {
  return first_status(
      batch_patch_device({DevRangePatch{key, offset, dev_ptr, length}}), key);
}

// A patch session's step: start by token, ONE launch (step_ladder), commit by
// token. nullopt: nothing was flipped or written and the session is dropped —
// the caller runs the full path, which may establish it again.
std::optional<Result<std::vector<int32_t>>> GpuClient::try_session_patch(
    const std::vector<DevRangePatch>& items, BatchPatchSession* sess) {
  if (!sess || sess->token == 0) return std::nullopt;
  // the session is bound to one item list, field by field
  bool same = sess->bound.size() == items.size();
  for (size_t i = 0; same && i < items.size(); ++i) {
    const auto& a = sess->bound[i];
    const auto& b = items[i];
    same = a.key == b.key && a.offset == b.offset && a.ptr == b.ptr &&
           a.length == b.length;
  }
  // a session that patches edge tiles lives only while the option is on
  if (!sess->edges.empty() && !patch_edge_tiles_) same = false;
  if (!same) {
    sess->end();
    return std::nullopt;
  }
  BB_TRACE_SCOPE("bb::session_patch");
  // RPC 1: the objects turn PENDING (placements pinned, epoch checked) and
  // the answer is what the keystone records for them now
  auto old = c_.patch_start_token(sess->token);
  if (!old.ok()) {  // nothing flipped
    sess->end();
    return std::nullopt;
  }
  auto keys_of = [&](auto pred) {
    std::vector<ObjectKey> keys;
    for (size_t i = 0; i < items.size(); ++i)
      if (pred(i)) keys.push_back(items[i].key);
    return keys;
  };
  auto all = [](size_t) { return true; };
  const uint32_t nshard = static_cast<uint32_t>(sess->shard_lens.size());
  const uint32_t nobj = static_cast<uint32_t>(sess->obj_sizes.size());
  if (old->obj_digests.size() != items.size() ||
      old->shard_digests.size() != nshard) {
    c_.patch_abort(keys_of(all));  // not what this session holds; unwritten
    sess->end();
    return std::nullopt;
  }
  // every copy is a kernel object of its own
  std::vector<uint64_t> obj_old(nobj);
  for (const auto& r : sess->ranges)
    for (uint32_t c = 0; c < r.ncopies; ++c)
      obj_old[r.first_obj + c] = old->obj_digests[r.item];
  const std::vector<uint64_t>& shard_old = old->shard_digests;
  // the patched keys leave the cache, as on the one-shot path
  cache_.erase(key_list(
      items, [](const DevRangePatch& it) -> const ObjectKey& { return it.key; }));

  const gpu::PatchSeg* segs = sess->segs.data();
  const uint32_t nseg = static_cast<uint32_t>(sess->segs.size());
  const gpu::PatchEdge* edges = sess->edges.data();
  const uint32_t nedge = static_cast<uint32_t>(sess->edges.size());
  const uint64_t* lens = sess->shard_lens.data();
  const uint64_t* sizes = sess->obj_sizes.data();
  std::vector<uint64_t> shard_new(nshard), obj_new(nobj);
  auto launched = step_ladder(
      sess->plan, sess->plan_failed, "patch ",
      [&](auto& p) {
        return p.build(segs, nseg, lens, nshard, sizes, nobj, device_, edges,
                       nedge);
      },
      [&](auto& p) {
        return p.run(shard_old.data(), obj_old.data(), shard_new.data(),
                     obj_new.data());
      },
      [&] {
        return gpu::fused_patch(segs, nseg, lens, shard_old.data(), nshard,
                                sizes, obj_old.data(), nobj, shard_new.data(),
                                obj_new.data(), streams_[2], edges, nedge);
      });
  std::vector<int32_t> statuses(items.size(), 0);
  auto torn = [&](ErrorCode code) {  // every key cancelled, the session over
    c_.cancel_puts(keys_of(all));
    statuses.assign(items.size(), static_cast<int32_t>(code));
    sess->end();
    return Result<std::vector<int32_t>>(std::move(statuses));
  };
  if (!launched.ok()) return {torn(launched.code())};

  std::vector<uint64_t> per_item(items.size());
  bool agree = true;
  for (const auto& r : sess->ranges) {
    per_item[r.item] = obj_new[r.first_obj];
    if (!copies_agree(obj_new, r)) {
      statuses[r.item] = static_cast<int32_t>(ErrorCode::CHECKSUM_MISMATCH);
      agree = false;
    }
  }
  if (!agree) {
    // diverged replicas: their keys are cancelled, the others commit by key
    std::vector<PutCompleteRequest> reqs;
    std::vector<uint32_t> order;
    for (const auto& r : sess->ranges) {
      if (statuses[r.item] != 0) continue;
      reqs.push_back(PutCompleteRequest{
          items[r.item].key, per_item[r.item],
          shard_digests_of(r, sess->copy_shards, shard_new)});
      order.push_back(r.item);
    }
    c_.cancel_puts(keys_of([&](size_t i) { return statuses[i] != 0; }));
    sess->end();
    if (auto r = c_.complete_by_keys(reqs, order, &statuses); !r.ok())
      return {r.error()};
    for (uint32_t i : order)
      if (statuses[i] == 0) ++patched_fused_items_;
    return {Result<std::vector<int32_t>>(std::move(statuses))};
  }
  // RPC 2: shards lie in item, copy, shard order — the wire order
  if (auto r = c_.commit_by_token_shards(sess->token, /*release=*/false,
                                         per_item.data(), per_item.size(),
                                         shard_new.data(), shard_new.size());
      !r.ok())
    return {torn(r.code())};
  session_patch_steps_.fetch_add(1);
  patched_fused_items_.fetch_add(items.size());
  return {Result<std::vector<int32_t>>(std::move(statuses))};
}

// ------------------------ compact v2 batch protocol ------------------------
// Pool-table responses with fixed-width placements: the client resolves each
// POOL once (not each object) and decodes with zero per-item allocations.

// The ladder of every session step: build the plan lazily, replay it, launch.
template <typename Plan, typename Build, typename Replay, typename Launch>
Result<void> GpuClient::step_ladder(std::shared_ptr<Plan>& plan,
                                    bool& plan_failed, const char* what,
                                    Build build, Replay replay, Launch launch) {
  static const bool no_graph = std::getenv("BB_NO_HIPGRAPH") != nullptr;
  if (!no_graph && !plan && !plan_failed) {
    auto built = std::make_shared<Plan>();
    auto rb = build(*built);
    if (rb.ok()) {
      plan = std::move(built);
    } else {
      plan_failed = true;       // capture unsupported: launch path
      (void)hipGetLastError();  // clear any sticky launch error
      BB_LOG(WARN) << what << "session graph capture unavailable ("
                   << rb.error().message << "); using per-op launches";
    }
  }
  if (plan) {
    auto r = replay(*plan);
    if (r.ok()) {
      session_graph_steps_.fetch_add(1);
      return r;
    }
    plan.reset();  // replay failed: fall through to launches
    plan_failed = true;
  }
  return launch();
}

// The launch of one session step, put or get, plain or striped.
Result<GpuClient::StepDigests> GpuClient::session_step(SessionCore& sess,
                                                       bool put) {
  auto run = [&](auto& plan, auto build, auto replay, auto launch) {
    return step_ladder(plan, sess.plan_failed, sess.striped() ? "striped " : "",
                       build, replay, launch);
  };
  StepDigests d;
  Result<void> r{};
  if (sess.striped()) {
    const gpu::StripeSeg* segs = sess.segs.data();
    const uint64_t* sizes = sess.obj_sizes.data();
    const uint32_t nseg = static_cast<uint32_t>(sess.segs.size());
    const uint32_t nobj = static_cast<uint32_t>(sess.obj_sizes.size());
    d.seg.assign(nseg, 0);
    d.obj.assign(nobj, 0);
    r = run(
        sess.stripe_plan,
        [&](auto& p) { return p.build(segs, nseg, sizes, nobj, device_); },
        [&](auto& p) { return p.run(d.seg.data(), d.obj.data()); },
        [&] {
          return gpu::fused_stripe(segs, nseg, sizes, nobj, d.seg.data(),
                                   d.obj.data(), streams_[2]);
        });
  } else {
    const gpu::PutDesc* descs = sess.descs.data();
    const uint32_t n = static_cast<uint32_t>(sess.descs.size());
    d.obj.assign(n, 0);
    r = run(
        sess.plan,
        [&](auto& p) { return p.build(descs, n, device_, warm_tail(put)); },
        [&](auto& p) { return p.run(d.obj.data()); },
        [&] {
          return gpu::fused_put(descs, n, d.obj.data(), streams_[2],
                                warm_tail(put));
        });
  }
  if (!r.ok()) return r.error();
  return d;
}

// A session's lists still describe `items`: item i owns the segments from
// its range to the next one's, each a slice of the item's buffer (the user
// side of the segment == ptr + first_tile tiles) of an object whose size
// fits size_ok(i, size). A plain desc is a segment at tile 0 of its own
// object: every copy of item i moves the whole buffer.
template <bool Put, typename Item, typename SizeOk>
static bool session_matches(const GpuClient::SessionCore& s,
                            const std::vector<Item>& items, SizeOk size_ok) {
  if (s.ranges.size() != items.size()) return false;
  auto user_of = [](const auto& seg) -> const void* {
    if constexpr (Put) return seg.src;
    else return seg.dst;
  };
  const bool striped = s.striped();
  for (size_t i = 0; i < items.size(); ++i) {
    const auto& r = s.ranges[i];
    if (!striped) {
      for (uint32_t k = r.first_seg; k < r.first_seg + r.ncopies; ++k)
        if (user_of(s.descs[k]) != items[i].ptr ||
            !size_ok(i, s.descs[k].nbytes))
          return false;
      continue;
    }
    for (uint32_t c = 0; c < r.ncopies; ++c)
      if (!size_ok(i, s.obj_sizes[r.first_obj + c])) return false;
    for (size_t k = r.first_seg, end = seg_end(s.ranges, i, s.segs.size());
         k < end; ++k) {
      const gpu::StripeSeg& seg = s.segs[k];
      if (seg.obj < r.first_obj || seg.obj >= r.first_obj + r.ncopies ||
          user_of(seg) != static_cast<const uint8_t*>(items[i].ptr) +
                              seg.first_tile * digest::kTileBytes)
        return false;
    }
  }
  return true;
}

// Token fast path: placements unchanged since last step ⇒ two tiny RPCs
// bracket ONE launch (session_step). Returns nullopt when the session is not
// usable (caller runs the full path, which re-establishes it).
std::optional<Result<std::vector<int32_t>>> GpuClient::try_session_put(
    const std::vector<DevPutItem>& items, BatchPutSession* sess,
    bool striped_route) {
  if (!sess || sess->striped() != striped_route || sess->token == 0 ||
      !cache_.owns(sess->binding) || items.empty())
    return std::nullopt;
  // the session is bound to one item list: same buffers, same order
  if (!cache_.valid(sess->binding) ||
      !session_matches<true>(*sess, items, [&](size_t i, uint64_t size) {
        return size == items[i].size;
      })) {
    sess->token = 0;
    return std::nullopt;
  }
  BB_TRACE_SCOPE(striped_route ? "bb::session_put_striped"
                               : "bb::session_put");
  // RPC 1 (8 bytes): flip the session's objects to PENDING — placements are
  // now pinned (tiering/eviction/repair only touch COMMITTED objects), so
  // the one-sided writes below cannot race a migration
  auto r1 = c_.meta_call_raw(M::BATCH_UPSERT_START,
                             wire::encode_upsert_start(sess->token));
  if (!r1.ok()) {
    sess->token = 0;  // stale/error before any write: clean fallback
    return std::nullopt;
  }
  auto step = session_step(*sess, /*put=*/true);
  if (!step.ok()) return {step.error()};  // objects stay PENDING; GC reclaims
  const StepDigests& d = step.value();
  std::vector<int32_t> statuses(items.size(), 0);
  // keep the session for the next step; one digest per ITEM, copy 0's, which
  // the plain form reads in place, its copies a fixed stride apart
  const uint64_t* digests = d.obj.data();
  size_t stride = sess->ranges[0].ncopies;
  std::vector<uint64_t> per_item;
  Result<void> r2{};
  if (!sess->striped()) {
    // (replicas hash identical bytes; they are not compared here)
    r2 = c_.commit_by_token(sess->token, /*release=*/false, digests,
                            items.size(), static_cast<uint32_t>(stride));
  } else {
    // A replica that disagrees saw the source change mid-step and must not
    // commit — as on the one-shot path its item fails and is cancelled; the
    // others commit by key, and the session ends.
    per_item.resize(items.size());
    bool agree = true;
    for (size_t i = 0; i < items.size(); ++i) {
      const auto& r = sess->ranges[i];
      per_item[i] = d.obj[r.first_obj];
      if (!copies_agree(d.obj, r)) {
        statuses[i] = static_cast<int32_t>(ErrorCode::TRANSFER_FAILED);
        agree = false;
      }
    }
    if (!agree) {
      sess->token = 0;
      std::vector<PutCompleteRequest> reqs;
      std::vector<uint32_t> order;
      for (size_t i = 0; i < items.size(); ++i) {
        if (statuses[i] != 0) continue;
        reqs.push_back(PutCompleteRequest{
            items[i].key, per_item[i],
            shard_digests_of(sess->ranges[i], sess->segs,
                             seg_end(sess->ranges, i, sess->segs.size()),
                             d.seg)});
        order.push_back(static_cast<uint32_t>(i));
      }
      if (auto r = c_.complete_by_keys(reqs, order, &statuses); !r.ok())
        return {r.error()};
      cancel_failed(items, statuses);
      return {Result<std::vector<int32_t>>(std::move(statuses))};
    }
    digests = per_item.data();
    stride = 1;
    // segments lie in item, copy, shard order: the wire order of the digests
    r2 = c_.commit_by_token_shards(sess->token, /*release=*/false, digests,
                                   items.size(), d.seg.data(), d.seg.size());
  }
  if (!r2.ok()) {
    // placements changed mid-step (rare): fall back — the full path
    // re-places and rewrites the batch
    sess->token = 0;
    return std::nullopt;
  }
  // refresh the cached digests so the verified get path accepts the new
  // contents (a binding that went stale meanwhile is simply not refreshed)
  (void)cache_.refresh_digests(sess->binding, digests, stride);
  session_put_steps_.fetch_add(1);
  return {Result<std::vector<int32_t>>(std::move(statuses))};
}

// What both put paths do with the placements they transferred.
template <typename Rebind>
void GpuClient::record_puts(const std::vector<PlacementCache::Put>& cached,
                            bool bind, uint64_t token, BatchPutSession* sess,
                            Rebind rebind) {
  PlacementCache::KeyList keys;
  if (bind)
    keys = key_list(cached, [](const PlacementCache::Put& p) -> const ObjectKey& {
      return p.key;
    });
  auto binding = cache_.record(cached, bind ? &keys : nullptr);
  if (!bind) return;
  sess->token = binding.bound() ? token : 0;
  if (binding.bound()) rebind(std::move(binding));
  else sess->rebind({}, 1, {});
}

Result<std::vector<int32_t>> GpuClient::batch_put_device_v2(
    const std::vector<DevPutItem>& items, const PlacementConfig& cfg,
    BatchPutSession* sess) {
  if (auto fast = try_session_put(items, sess, /*striped_route=*/false))
    return std::move(*fast);
  BB_TRACE_SCOPE("bb::batch_put");
  // establish: a reusable session for upsert steps (token kept server-side;
  // replicated single-shard placements qualify — one desc per copy)
  const bool establish = sess != nullptr && cfg.replace && cfg.checksum &&
                         fused_copy_ && cache_.enabled();
  // one-shot tokens let ANY all-fused batch commit by token+digests instead
  // of re-sending every key in BATCH_PUT_COMPLETE (released at commit)
  const bool want_token = establish || (cfg.checksum && fused_copy_);
  const uint32_t dpi = std::max<uint32_t>(cfg.replication, 1);
  auto resp = c_.meta_call_raw(
      M::BATCH_PUT_START2,
      wire::encode_put_start2_request(items, cfg, want_token));
  if (!resp.ok()) return resp.error();
  wire::BatchPlacements pl;
  BB_RETURN_IF_ERROR(
      wire::decode_put_start2_response(resp.value(), items.size(), pl));
  const uint64_t token = pl.token;  // 0 = no session granted
  const auto pools = resolve_pools(pl.pools);

  std::vector<int32_t> statuses(items.size(), 0);
  Router<true> rt(*this, fused_copy_, /*defer=*/true);
  std::vector<PlacementCache::Put> cached;  // hashed items, digest filled later

  for (size_t i = 0; i < items.size(); ++i) {
    const wire::ItemPlaces& ip = pl.items[i];
    if (ip.status != 0) {  // placement error
      statuses[i] = ip.status;
      continue;
    }
    const wire::Place* places = pl.places_of(ip);
    const uint8_t* isrc = static_cast<const uint8_t*>(items[i].ptr);
    // fused copy+digest fast path: every copy base-resolvable + aligned
    // (one desc per copy, digests identical across replicas)
    bool all_fusable =
        fused_copy_ && cfg.checksum && ip.ncopies == dpi && aligned16(isrc);
    for (uint8_t c = 0; c < ip.ncopies && all_fusable; ++c)
      all_fusable =
          places[c].pool_idx < pools.size() && pools[places[c].pool_idx].base &&
          aligned16(pools[places[c].pool_idx].base + places[c].offset);
    if (all_fusable) {
      for (uint8_t c = 0; c < ip.ncopies; ++c) {
        const PoolRef& pr = pools[places[c].pool_idx];
        rt.hashed.push_back({isrc, pr.base + places[c].offset, items[i].size});
        if (c == 0)  // the verified-get cache reads copy 0
          cached.push_back({items[i].key,
                            {pr.pool_id, places[c].offset, items[i].size, 0}});
      }
      rt.hashed_idx.push_back(static_cast<uint32_t>(i));
      continue;
    }
    // general route; a copy naming a pool outside the table fails the item
    bool ok = true;
    for (uint8_t c = 0; c < ip.ncopies && ok; ++c)
      ok = places[c].pool_idx < pools.size() &&
           rt.add(isrc, pools[places[c].pool_idx], places[c].offset,
                  items[i].size, static_cast<uint32_t>(i)).ok();
    if (ok) rt.plain_idx.push_back(static_cast<uint32_t>(i));
    else statuses[i] = static_cast<int32_t>(ErrorCode::TRANSFER_FAILED);
  }
  // unmappable pools (direct-IO NVMe tier, TCP-only remotes): fan the staged
  // writes out on a side thread so the disk overlaps the kernel launches and
  // digest passes below
  std::future<Result<void>> staged_fut;
  if (!rt.staged.empty())
    staged_fut = std::async(std::launch::async, [&] {
      (void)hipSetDevice(device_);
      return staged_write_many(rt.staged);
    });
  BB_RETURN_IF_ERROR(rt.launch_put(items, cfg.checksum));
  if (staged_fut.valid()) {
    auto r = staged_fut.get();
    if (!r.ok())  // failed staged items must not commit (cancelled below)
      for (auto i : rt.staged_idx)
        statuses[i] = static_cast<int32_t>(ErrorCode::TRANSFER_FAILED);
  }
  const bool all_hashed = rt.hashed_idx.size() == items.size();

  // commit: token path (8 B + digests, no key strings) when the whole batch
  // rode the fused single-copy path (one-shot tokens are released by the
  // commit); key-based BATCH_PUT_COMPLETE otherwise, or if the token went
  // stale (concurrent placement change)
  const bool committed_by_token =
      token != 0 && all_hashed &&
      c_.commit_by_token(token, /*release=*/!establish,
                         rt.hashed_digests.data(), items.size(), dpi).ok();
  if (!committed_by_token)
    BB_RETURN_IF_ERROR(complete_puts(items, rt, dpi, nullptr, statuses,
                                     /*apply_statuses=*/false));
  if (!cached.empty() && cache_.enabled()) {
    // remember our own single-copy placements + digests for RPC-free
    // verified gets (see set_placement_cache)
    for (size_t j = 0; j < cached.size(); ++j)
      cached[j].entry.digest = rt.hashed_digests[j * dpi];
    // establish the batch session when the server granted a token AND every
    // item rode the fused single-copy path (so desc j == item j) AND every
    // key is cached after recording
    const bool bind = sess && establish && token != 0 && all_hashed;
    record_puts(cached, bind, token, sess, [&](PlacementCache::Binding b) {
      sess->rebind(rt.hashed, dpi, std::move(b));
    });
  }
  cancel_failed(items, statuses);
  return statuses;
}

// ----------------------------------------------- verified placement cache

void GpuClient::invalidate(const std::vector<ObjectKey>& keys) {
  cache_.erase(key_list(
      keys, [](const ObjectKey& k) -> const ObjectKey& { return k; }));
}

Result<void> GpuClient::refetch(const std::vector<DevGetItem>& items,
                                const std::vector<uint32_t>& idx, bool verify,
                                std::vector<int32_t>& statuses) {
  std::vector<DevGetItem> sub;
  sub.reserve(idx.size());
  for (auto i : idx) sub.push_back(items[i]);
  auto r = batch_get_device_rpc(sub, verify);
  if (!r.ok()) return r.error();
  for (size_t j = 0; j < idx.size(); ++j) statuses[idx[j]] = r.value()[j];
  return {};
}

// Session fast path for gets: descs and want-digest slots were resolved on a
// previous step; a step is ONE kernel launch + digest compares, zero RPCs.
std::optional<Result<std::vector<int32_t>>> GpuClient::try_session_get(
    const std::vector<DevGetItem>& items, BatchGetSession* sess) {
  if (!sess || !sess->complete || !cache_.owns(sess->binding) || items.empty())
    return std::nullopt;
  std::vector<uint64_t> want(items.size());
  if (!cache_.read_digests(sess->binding, want.data(), want.size()) ||
      !session_matches<false>(*sess, items, [&](size_t i, uint64_t size) {
        return size <= items[i].capacity;
      })) {
    sess->complete = false;
    return std::nullopt;
  }
  BB_TRACE_SCOPE(sess->striped() ? "bb::session_get_striped"
                                 : "bb::session_get");
  auto step = session_step(*sess, /*put=*/false);
  if (!step.ok()) return {step.error()};
  // copy 0's object digest of every item against the cached one
  const std::vector<uint64_t>& got = step.value().obj;
  std::vector<uint32_t> miss;
  for (size_t j = 0; j < items.size(); ++j)
    if (got[sess->ranges[j].first_obj] != want[j])
      miss.push_back(static_cast<uint32_t>(j));
  if (!miss.empty()) return {refetch_stale(items, miss, *sess)};
  session_get_steps_.fetch_add(1);
  return {Result<std::vector<int32_t>>(std::vector<int32_t>(items.size(), 0))};
}

// Stale entries: drop them (which ends every session on this cache) and
// refetch the misses authoritatively.
Result<std::vector<int32_t>> GpuClient::refetch_stale(
    const std::vector<DevGetItem>& items, const std::vector<uint32_t>& miss,
    BatchGetSession& sess) {
  cache_.erase(key_list(miss, [&](uint32_t j) -> const ObjectKey& {
    return items[j].key;
  }));
  sess.complete = false;
  std::vector<int32_t> statuses(items.size(), 0);
  BB_RETURN_IF_ERROR(refetch(items, miss, /*verify=*/true, statuses));
  return statuses;
}

Result<std::vector<int32_t>> GpuClient::batch_get_device_v2(
    const std::vector<DevGetItem>& items, bool verify, BatchGetSession* sess) {
  if (auto fast = try_session_get(items, sess)) return std::move(*fast);
  if (!cache_.enabled_and_nonempty()) return batch_get_device_rpc(items, verify);

  // optimistic leg: one-sided reads of cached placements through the
  // copy+digest kernel; a digest mismatch (moved/replaced/evicted object)
  // demotes the key to the RPC leg and drops the cache entry
  std::vector<PlacementCache::Want> wants;
  wants.reserve(items.size());
  for (const auto& it : items) wants.push_back({it.key, it.capacity});
  auto lk = cache_.lookup(wants);
  std::vector<uint32_t> miss_idx = lk.misses;
  // pool resolution may RPC (view-versioned pool cache) — outside the lock
  std::vector<gpu::PutDesc> descs;
  std::vector<uint32_t> hit_idx;
  std::vector<uint64_t> want;
  StripeBatch stripes;  // hits on striped entries: verified by object digest
  std::vector<uint64_t> stripe_want;
  for (const auto& [i, cp] : lk.hits) {
    if (!cp.shards.empty()) {
      if (fused_copy_ && aligned16(items[i].ptr) &&
          stripes.add_cached<false>(*this, static_cast<uint8_t*>(items[i].ptr),
                                    cp)) {
        stripes.entries.push_back(
            {i, static_cast<uint32_t>(stripes.obj_sizes.size() - 1), 1,
             static_cast<uint32_t>(stripes.segs.size() - cp.shards.size())});
        stripe_want.push_back(cp.digest);
      } else {
        miss_idx.push_back(i);
      }
      continue;
    }
    uint8_t* base = resolve_pool_base(cp.pool_id);
    if (base && aligned16(items[i].ptr, base + cp.offset)) {
      descs.push_back(
          {base + cp.offset, static_cast<uint8_t*>(items[i].ptr), cp.size});
      hit_idx.push_back(i);
      want.push_back(cp.digest);
    } else {
      miss_idx.push_back(i);
    }
  }
  std::vector<int32_t> statuses(items.size(), 0);
  if (!descs.empty() || !stripes.entries.empty()) {
    BB_TRACE_SCOPE("bb::cached_get");
    std::vector<uint64_t> got(descs.size(), 0);
    auto r = gpu::fused_put(descs.data(), static_cast<uint32_t>(descs.size()),
                            got.data(), streams_[2], warm_tail(/*put=*/false));
    if (!r.ok()) return r.error();
    BB_RETURN_IF_ERROR(stripes.run(streams_[2]));
    striped_fused_get_items_.fetch_add(stripes.entries.size());
    // digest mismatches join the misses (refetched authoritatively); their
    // keys are the stale ones
    const size_t first_stale = miss_idx.size();
    for (size_t j = 0; j < hit_idx.size(); ++j)
      if (got[j] != want[j]) miss_idx.push_back(hit_idx[j]);
    for (size_t j = 0; j < stripes.entries.size(); ++j)
      if (stripes.obj_digests[stripes.entries[j].first_obj] != stripe_want[j])
        miss_idx.push_back(stripes.entries[j].item);
    const auto stale = key_list(
        std::span<const uint32_t>(miss_idx).subspan(first_stale),
        [&](uint32_t i) -> const ObjectKey& { return items[i].key; });
    // establish the get session when every item was a verified cache hit of
    // ONE kind (desc j == item j, or striped range j == item j; a mixed
    // batch gets none) and no concurrent thread mutated the cache
    const bool all_plain = hit_idx.size() == items.size();
    const bool all_striped = stripes.entries.size() == items.size();
    auto binding =
        cache_.settle(std::move(lk), stale, sess && (all_plain || all_striped));
    if (binding.bound()) {
      if (all_striped)
        sess->rebind_striped(std::move(stripes.segs),
                             std::move(stripes.obj_sizes),
                             std::move(stripes.entries), std::move(binding));
      else
        sess->rebind(std::move(descs), /*copies=*/1, std::move(binding));
      sess->complete = true;
    }
  }
  if (!miss_idx.empty()) {
    std::sort(miss_idx.begin(), miss_idx.end());
    BB_RETURN_IF_ERROR(refetch(items, miss_idx, verify, statuses));
  }
  return statuses;
}

Result<std::vector<int32_t>> GpuClient::batch_get_device_rpc(
    const std::vector<DevGetItem>& items, bool verify) {
  BB_TRACE_SCOPE("bb::batch_get");
  auto resp = c_.meta_call_raw(M::BATCH_GET_WORKERS2,
                               wire::encode_get_workers2_request(items));
  if (!resp.ok()) return resp.error();
  wire::BatchPlacements pl;
  BB_RETURN_IF_ERROR(
      wire::decode_get_workers2_response(resp.value(), items.size(), pl));
  const auto pools = resolve_pools(pl.pools);

  std::vector<int32_t> statuses(items.size(), 0);
  Router<false> rt(*this, fused_copy_, /*defer=*/true);
  for (size_t i = 0; i < items.size(); ++i) {
    const wire::ItemPlaces& ip = pl.items[i];
    if (ip.status != 0) {
      statuses[i] = ip.status;
      continue;
    }
    if (ip.size > items[i].capacity) {
      statuses[i] = static_cast<int32_t>(ErrorCode::SIZE_MISMATCH);
      continue;
    }
    uint8_t* dst = static_cast<uint8_t*>(items[i].ptr);
    bool done = false;
    Error last{ErrorCode::NO_PLACEMENT, "no copies"};
    for (uint8_t c = 0; c < ip.ncopies && !done; ++c) {
      const wire::Place& p = pl.places_of(ip)[c];
      if (p.pool_idx >= pools.size()) continue;  // unknown pool: skip copy
      const PoolRef& pr = pools[p.pool_idx];
      // verify mode: the gather rides the copy+digest kernel, so
      // verification costs no extra read of the data
      if (pr.base && fused_copy_ && verify && ip.checksum != 0 &&
          aligned16(dst, pr.base + p.offset)) {
        rt.hashed.push_back({pr.base + p.offset, dst, ip.size});
        rt.hashed_idx.push_back(static_cast<uint32_t>(i));
        done = true;
        continue;
      }
      // (a staged copy counts as fetched: completion is checked after the
      // fan-out below)
      auto r = rt.add(dst, pr, p.offset, ip.size, static_cast<uint32_t>(i));
      if (r.ok()) {
        rt.plain_idx.push_back(static_cast<uint32_t>(i));
        done = true;
      } else {
        last = r.error();
      }
    }
    if (!done) statuses[i] = static_cast<int32_t>(last.code);
  }
  if (!rt.staged.empty()) {
    auto r = staged_read_many(rt.staged);
    if (!r.ok())
      // mark the whole staged group failed (partial data is not returned)
      for (auto i : rt.staged_idx) statuses[i] = static_cast<int32_t>(r.code());
  }
  BB_RETURN_IF_ERROR(rt.finish_get(
      items, verify,
      [&](uint32_t i) {
        return std::make_pair(pl.items[i].size, pl.items[i].checksum);
      },
      statuses));
  return statuses;
}

// -------------------------------------------------------------- batch ops

Result<std::vector<int32_t>> GpuClient::batch_put_device(
    const std::vector<DevPutItem>& items, const PlacementConfig& cfg,
    BatchPutSession* sess) {
  // keystone failover mid-batch: the new leader never saw this batch's
  // PENDING state — the failover-shaped failures are redone once
  return c_.redo_after_failover(items, [&](const auto& its, bool first) {
    return batch_put_device_once(its, cfg, first ? sess : nullptr);
  });
}

Result<std::vector<int32_t>> GpuClient::batch_put_device_once(
    const std::vector<DevPutItem>& items, const PlacementConfig& cfg,
    BatchPutSession* sess) {
  BB_RETURN_IF_ERROR(init());
  BB_HIP_TRY(hipSetDevice(device_));
  if (cfg.max_workers_per_copy <= 1)
    return batch_put_device_v2(items, cfg, sess);

  if (auto fast = try_session_put(items, sess, /*striped_route=*/true))
    return std::move(*fast);
  BatchPutStartRequest breq;
  breq.requests.reserve(items.size());
  for (const auto& it : items)
    breq.requests.push_back(PutStartRequest{it.key, it.size, cfg});
  auto start = c_.meta_call<BatchPutStartRequest, BatchPutStartResponse>(
      M::BATCH_PUT_START, breq);
  if (!start.ok()) return start.error();

  std::vector<int32_t> statuses(items.size(), 0);
  Router<true> rt(*this, fused_copy_, /*defer=*/false);
  StripeBatch stripes;

  for (size_t i = 0; i < items.size(); ++i) {
    auto& placed = start->items[i];
    if (placed.status != 0) {
      statuses[i] = placed.status;
      continue;
    }
    // fast path: single device-visible shard + digest wanted → ONE fused
    // copy+hash kernel reads the object once
    if (fused_copy_ && cfg.checksum && placed.copies.size() == 1 &&
        placed.copies[0].shards.size() == 1) {
      uint8_t* dst = resolve_device_ptr(placed.copies[0].shards[0]);
      if (dst && aligned16(items[i].ptr, dst)) {
        rt.hashed.push_back({items[i].ptr, dst, items[i].size});
        rt.hashed_idx.push_back(static_cast<uint32_t>(i));
        continue;
      }
    }
    // striped fast path: every shard of every copy device-visible and on a
    // tile boundary of the object → the item rides the fused_stripe launch
    // (copy, per-shard digests and object digest from one read)
    if (fused_copy_ && cfg.checksum && aligned16(items[i].ptr)) {
      const size_t seg_mark = stripes.segs.size();
      const size_t obj_mark = stripes.obj_sizes.size();
      bool all = any_striped(placed.copies);
      for (size_t c = 0; c < placed.copies.size() && all; ++c)
        all = stripes.add_copy<true>(*this,
                                     static_cast<const uint8_t*>(items[i].ptr),
                                     items[i].size, placed.copies[c]);
      if (all) {
        stripes.entries.push_back({static_cast<uint32_t>(i),
                                   static_cast<uint32_t>(obj_mark),
                                   static_cast<uint32_t>(placed.copies.size()),
                                   static_cast<uint32_t>(seg_mark)});
        continue;
      }
      stripes.rewind(seg_mark, obj_mark);
    }
    bool ok = true;
    for (const auto& copy : placed.copies)
      if (!(ok = rt.add_copy(static_cast<const uint8_t*>(items[i].ptr), copy,
                             static_cast<uint32_t>(i)).ok()))
        break;
    if (ok) rt.plain_idx.push_back(static_cast<uint32_t>(i));
    else statuses[i] = static_cast<int32_t>(ErrorCode::TRANSFER_FAILED);
  }
  BB_RETURN_IF_ERROR(rt.launch_put(items, cfg.checksum));
  BB_RETURN_IF_ERROR(stripes.run(streams_[2]));

  // per-shard digests for striped copies that took the general route (one
  // batched launch hashes every source slice) — recorded server-side so the scrubber can verify each
  // striped shard independently
  std::map<uint32_t, std::vector<std::vector<uint64_t>>> shard_digests;
  if (cfg.checksum) {
    struct Slot {
      uint32_t item, copy, shard;
      const void* ptr;
      uint64_t size;
    };
    std::vector<Slot> slots;
    std::vector<uint32_t> slot_idx;
    for (auto i : rt.plain_idx) {
      const auto& copies = start->items[i].copies;
      if (!any_striped(copies)) continue;
      auto& out = shard_digests[i];
      out.resize(copies.size());
      for (uint32_t c = 0; c < copies.size(); ++c) {
        out[c].resize(copies[c].shards.size(), 0);
        uint64_t off = 0;
        for (uint32_t s2 = 0; s2 < copies[c].shards.size(); ++s2) {
          slot_idx.push_back(static_cast<uint32_t>(slots.size()));
          slots.push_back({i, c, s2,
                           static_cast<const uint8_t*>(items[i].ptr) + off,
                           copies[c].shards[s2].length});
          off += copies[c].shards[s2].length;
        }
      }
    }
    auto got = digest_items(
        slot_idx, [&](uint32_t k) { return slots[k].ptr; },
        [&](uint32_t k) { return slots[k].size; }, streams_[1]);
    if (!got.ok()) return got.error();
    for (size_t k = 0; k < slots.size(); ++k)
      shard_digests[slots[k].item][slots[k].copy][slots[k].shard] =
          got.value()[k];
  }

  // the fused_stripe items complete with the plain group: the object digest
  // is copy 0's (replicas hashed the same source; one that disagrees saw it
  // change mid-batch and must not commit), the shard digests are the
  // launch's segment digests in copy, shard order
  for (const auto& e : stripes.entries) {
    if (!copies_agree(stripes.obj_digests, e))
      statuses[e.item] = static_cast<int32_t>(ErrorCode::TRANSFER_FAILED);
    shard_digests[e.item] = shard_digests_of(e, start->items[e.item].copies,
                                             stripes.seg_digests);
    rt.plain_idx.push_back(e.item);
    rt.plain_digests.push_back(stripes.obj_digests[e.first_obj]);
  }
  striped_fused_items_.fetch_add(stripes.entries.size());

  // establish a striped session when EVERY item rode the fused_stripe launch
  // (range j == item j). The server session is opened NOW: the objects are
  // still PENDING, which pins the placements just resolved — after the
  // commit a migration could make the session "current" over addresses this
  // client no longer has right.
  const bool all_striped = !items.empty() &&
                           stripes.entries.size() == items.size() &&
                           std::all_of(statuses.begin(), statuses.end(),
                                       [](int32_t st) { return st == 0; });
  uint64_t token = 0;
  if (sess && cfg.replace && cfg.checksum && fused_copy_ && cache_.enabled() &&
      all_striped) {
    std::vector<std::pair<ObjectKey, uint64_t>> objects;
    objects.reserve(items.size());
    for (const auto& it : items) objects.emplace_back(it.key, it.size);
    if (auto t = c_.open_session(objects, /*allow_striped=*/true); t.ok())
      token = t.value();
  }
  // all striped: rt.plain_digests holds exactly the items' object digests,
  // and the segments lie in item, copy, shard order — the wire order
  const bool committed_by_token =
      token != 0 &&
      c_.commit_by_token_shards(token, /*release=*/false,
                                rt.plain_digests.data(), items.size(),
                                stripes.seg_digests.data(),
                                stripes.seg_digests.size()).ok();
  if (!committed_by_token)
    BB_RETURN_IF_ERROR(complete_puts(items, rt, 1, &shard_digests, statuses,
                                     /*apply_statuses=*/true));
  if (!stripes.entries.empty() && cache_.enabled()) {
    // remember copy 0 of every committed fused-striped item for RPC-free
    // verified gets; with a session, bind it over all of them
    std::vector<PlacementCache::Put> cached;
    for (const auto& e : stripes.entries) {
      if (statuses[e.item] != 0) continue;
      const auto& shards = start->items[e.item].copies[0].shards;
      PlacementCache::Entry ce{shards[0].pool_id, shards[0].offset,
                               items[e.item].size,
                               stripes.obj_digests[e.first_obj], {}};
      for (const auto& s : shards)
        ce.shards.push_back({s.pool_id, s.offset, s.length});
      cached.push_back({items[e.item].key, std::move(ce)});
    }
    const bool bind = committed_by_token && cached.size() == items.size();
    record_puts(cached, bind, token, sess, [&](PlacementCache::Binding b) {
      sess->rebind_striped(std::move(stripes.segs),
                           std::move(stripes.obj_sizes),
                           std::move(stripes.entries), std::move(b));
    });
  }
  cancel_failed(items, statuses);
  return statuses;
}

Result<std::vector<int32_t>> GpuClient::batch_get_device(
    const std::vector<DevGetItem>& items, bool verify, BatchGetSession* sess) {
  return c_.redo_after_failover(items, [&](const auto& its, bool first) {
    return batch_get_device_once(its, verify, first ? sess : nullptr);
  });
}

Result<std::vector<int32_t>> GpuClient::batch_get_device_once(
    const std::vector<DevGetItem>& items, bool verify, BatchGetSession* sess) {
  BB_RETURN_IF_ERROR(init());
  BB_HIP_TRY(hipSetDevice(device_));
  {
    auto v2 = batch_get_device_v2(items, verify, sess);
    // a striped object in the batch makes the server signal fallback per
    // item; only a whole-response failure falls back to v1
    if (v2.ok()) {
      bool any_fallback = false;
      for (auto st : v2.value())
        if (st == static_cast<int32_t>(ErrorCode::NOT_IMPLEMENTED))
          any_fallback = true;
      if (!any_fallback) return v2;
    }
  }

  KeysMsg req;
  for (const auto& it : items) req.keys.push_back(it.key);
  auto meta = c_.meta_call<KeysMsg, BatchGetWorkersResponse>(
      M::BATCH_GET_WORKERS, req);
  if (!meta.ok()) return meta.error();

  std::vector<int32_t> statuses(items.size(), 0);
  Router<false> rt(*this, fused_copy_, /*defer=*/false);
  StripeBatch stripes;

  for (size_t i = 0; i < items.size(); ++i) {
    auto& item = meta->items[i];
    if (item.status != 0) {
      statuses[i] = item.status;
      continue;
    }
    if (item.info.size > items[i].capacity) {
      statuses[i] = static_cast<int32_t>(ErrorCode::SIZE_MISMATCH);
      continue;
    }
    // verified get of a striped copy: gathered AND hashed by the
    // fused_stripe launch, so verification costs no second read
    const bool stripe_ok = verify && fused_copy_ && item.info.checksum != 0 &&
                           aligned16(items[i].ptr);
    bool ok = false, striped = false;
    for (const auto& copy : item.info.copies) {
      if (stripe_ok && copy.shards.size() > 1 &&
          stripes.add_copy<false>(*this, static_cast<uint8_t*>(items[i].ptr),
                                  item.info.size, copy)) {
        stripes.entries.push_back(
            {static_cast<uint32_t>(i),
             static_cast<uint32_t>(stripes.obj_sizes.size() - 1), 1, 0});
        ok = striped = true;
        break;
      }
      if ((ok = rt.add_copy(static_cast<uint8_t*>(items[i].ptr), copy,
                            static_cast<uint32_t>(i)).ok()))
        break;  // first healthy copy wins
    }
    if (striped) continue;
    if (ok) rt.plain_idx.push_back(static_cast<uint32_t>(i));
    else statuses[i] = static_cast<int32_t>(ErrorCode::TRANSFER_FAILED);
  }
  BB_RETURN_IF_ERROR(stripes.run(streams_[2]));
  for (const auto& e : stripes.entries)
    if (stripes.obj_digests[e.first_obj] != meta->items[e.item].info.checksum)
      statuses[e.item] = static_cast<int32_t>(ErrorCode::CHECKSUM_MISMATCH);
  striped_fused_get_items_.fetch_add(stripes.entries.size());
  BB_RETURN_IF_ERROR(rt.finish_get(
      items, verify,
      [&](uint32_t i) {
        return std::make_pair(meta->items[i].info.size,
                              meta->items[i].info.checksum);
      },
      statuses));
  return statuses;
}

// --------------------------------------------------- collective shuffle

Result<void> GpuClient::batch_shuffle_rccl(RcclEngine& comm,
                                           const std::vector<ShuffleWant>& want) {
  BB_RETURN_IF_ERROR(init());
  BB_HIP_TRY(hipSetDevice(device_));
  RcclExchanger ex(comm, streams_[3]);
  GpuCopier cp(device_, streams_[4]);
  // serve keys out of this rank's visible pools: placement cache first
  // (covers this client's own puts), metadata RPC as the general fallback
  ShuffleResolver resolve = [this](const ObjectKey& key,
                                   uint64_t size) -> const void* {
    if (auto cp2 = cache_.find(key);
        cp2 && cp2->size == size && cp2->shards.empty()) {
      // resolve_pool_base may RPC — the cache lock is not held here
      if (uint8_t* base = resolve_pool_base(cp2->pool_id))
        return base + cp2->offset;
      return nullptr;
    }
    auto meta = c_.meta_call<KeyMsg, GetWorkersResponse>(M::GET_WORKERS,
                                                         KeyMsg{key});
    if (!meta.ok() || meta->size != size) return nullptr;
    for (const auto& copy : meta->copies) {
      if (copy.shards.size() != 1) continue;
      if (uint8_t* p = resolve_device_ptr(copy.shards[0])) return p;
    }
    return nullptr;
  };
  return batch_shuffle(ex, cp, resolve, want);
}

// ------------------------------------------------------- pipelined batches

template <typename Fn>
Result<uint64_t> GpuClient::submit_async(Fn fn) {
  if (!initialized_) BB_RETURN_IF_ERROR(init());
  std::lock_guard<std::mutex> g(async_mu_);
  uint64_t token = next_async_++;
  async_[token] = std::async(std::launch::async, [this, fn = std::move(fn)] {
    (void)hipSetDevice(device_);
    return fn();
  });
  return token;
}

Result<uint64_t> GpuClient::batch_put_async(std::vector<DevPutItem> items,
                                            PlacementConfig cfg) {
  return submit_async([this, items = std::move(items), cfg] {
    return batch_put_device(items, cfg);
  });
}

Result<uint64_t> GpuClient::batch_get_async(std::vector<DevGetItem> items,
                                            bool verify) {
  return submit_async([this, items = std::move(items), verify] {
    return batch_get_device(items, verify);
  });
}

Result<std::vector<int32_t>> GpuClient::async_wait(uint64_t token) {
  std::future<Result<std::vector<int32_t>>> f;
  {
    std::lock_guard<std::mutex> g(async_mu_);
    auto it = async_.find(token);
    if (it == async_.end())
      return Error{ErrorCode::INVALID_ARGUMENT,
                   "unknown async batch token " + std::to_string(token)};
    f = std::move(it->second);
    async_.erase(it);
  }
  return f.get();
}

}  // namespace blackbird
