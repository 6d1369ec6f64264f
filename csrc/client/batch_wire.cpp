#include "blackbird/client/batch_wire.h"

namespace blackbird::wire {

namespace {
Error bad(const char* what) { return Error{ErrorCode::PROTOCOL_ERROR, what}; }

void encode_pools(serde::Enc& e, const std::vector<PoolId>& pools) {
  e.num<uint16_t>(static_cast<uint16_t>(pools.size()));
  for (auto& p : pools) e.str(p);
}

void encode_items(serde::Enc& e, const BatchPlacements& p, bool get) {
  for (auto& it : p.items) {
    e.num<uint8_t>(it.status == 0 ? 0 : 1);
    if (it.status != 0) {
      e.num<int32_t>(it.status);
      continue;
    }
    if (get) {
      e.num<uint64_t>(it.size);
      e.num<uint64_t>(it.checksum);
    }
    e.num<uint8_t>(it.ncopies);
    for (uint8_t c = 0; c < it.ncopies; ++c) {
      e.num<uint16_t>(p.places[it.first_place + c].pool_idx);
      e.num<uint64_t>(p.places[it.first_place + c].offset);
    }
  }
}

Result<void> decode_response(serde::Dec& d, size_t nitems, bool get,
                             BatchPlacements& out) {
  const uint16_t npools = d.num<uint16_t>();
  out.pools.clear();
  for (uint16_t i = 0; i < npools && d.ok(); ++i) out.pools.push_back(d.str());
  out.items.clear();
  out.places.clear();
  for (size_t i = 0; i < nitems && d.ok(); ++i) {
    ItemPlaces it;
    if (d.num<uint8_t>() != 0) {
      it.status = d.num<int32_t>();
    } else {
      if (get) {
        it.size = d.num<uint64_t>();
        it.checksum = d.num<uint64_t>();
      }
      it.ncopies = d.num<uint8_t>();
      it.first_place = static_cast<uint32_t>(out.places.size());
      for (uint8_t c = 0; c < it.ncopies && d.ok(); ++c) {
        const uint16_t pi = d.num<uint16_t>();
        out.places.push_back({pi, d.num<uint64_t>()});
      }
    }
    out.items.push_back(it);
  }
  if (!d.ok()) return bad("bad v2 response");
  return {};
}

// every key costs at least its 4 length bytes: a count the body cannot hold
// is rejected before anything is sized by it
bool count_fits(uint32_t count, const serde::Dec& d) {
  return d.ok() && static_cast<uint64_t>(count) * 4 <= d.remaining();
}

// u32 n | u64*n: the list is sized only once the body is known to hold it
void encode_u64_list(serde::Enc& e, const uint64_t* v, size_t n) {
  e.num<uint32_t>(static_cast<uint32_t>(n));
  for (size_t i = 0; i < n; ++i) e.num<uint64_t>(v[i]);
}
bool decode_u64_list(serde::Dec& d, std::vector<uint64_t>& out) {
  const uint32_t n = d.num<uint32_t>();
  if (!d.ok() || n > (1u << 24) || d.remaining() < n * sizeof(uint64_t))
    return false;
  out.resize(n);
  for (auto& v : out) v = d.num<uint64_t>();
  return true;
}
}  // namespace

std::string encode_upsert_start(uint64_t token) {
  serde::Enc e;
  e.num<uint64_t>(token);
  return std::move(e.buf);
}

std::string encode_commit_token(uint64_t token, bool release,
                                const uint64_t* digests, size_t n,
                                size_t stride) {
  serde::Enc e;
  e.num<uint64_t>(token);
  e.num<uint8_t>(release ? 1 : 0);
  e.num<uint32_t>(static_cast<uint32_t>(n));
  for (size_t i = 0; i < n; ++i) e.num<uint64_t>(digests[i * stride]);
  return std::move(e.buf);
}

Result<PutStart2Request> decode_put_start2_request(const std::string& body) {
  serde::Dec d(body.data(), body.size());
  PutStart2Request r;
  const uint32_t count = d.num<uint32_t>();
  const uint64_t uniform = d.num<uint64_t>();
  if (!count_fits(count, d)) return bad("bad v2 request");
  r.sizes.assign(count, uniform);
  if (uniform == 0)
    for (auto& s : r.sizes) s = d.num<uint64_t>();
  r.keys.resize(count);
  for (auto& k : r.keys) k = d.str();
  serde::get(d, r.cfg);
  r.want_token = d.remaining() ? d.num<uint8_t>() : 0;
  if (!d.ok()) return bad("bad v2 request");
  return r;
}

Result<std::vector<ObjectKey>> decode_get_workers2_request(
    const std::string& body) {
  serde::Dec d(body.data(), body.size());
  const uint32_t count = d.num<uint32_t>();
  if (!count_fits(count, d)) return bad("bad v2 request");
  std::vector<ObjectKey> keys(count);
  for (auto& k : keys) k = d.str();
  if (!d.ok()) return bad("bad v2 request");
  return keys;
}

Result<uint64_t> decode_upsert_start(const std::string& body) {
  serde::Dec d(body.data(), body.size());
  const uint64_t token = d.num<uint64_t>();
  if (!d.ok()) return bad("bad upsert request");
  return token;
}

Result<CommitToken> decode_commit_token(const std::string& body) {
  serde::Dec d(body.data(), body.size());
  CommitToken c;
  c.token = d.num<uint64_t>();
  c.flags = d.num<uint8_t>();
  const uint32_t n = d.num<uint32_t>();
  if (!d.ok() || d.remaining() != n * sizeof(uint64_t) || n > (1u << 24))
    return bad("bad commit request");
  c.digests.resize(n);
  for (auto& dg : c.digests) dg = d.num<uint64_t>();
  return c;
}

std::string encode_session_open_response(uint64_t token) {
  return encode_upsert_start(token);  // both are one u64
}

std::string encode_commit_token_shards(uint64_t token, bool release,
                                       const uint64_t* obj_digests, size_t n,
                                       const uint64_t* shard_digests,
                                       size_t m) {
  serde::Enc e;
  e.num<uint64_t>(token);
  e.num<uint8_t>(release ? 1 : 0);
  encode_u64_list(e, obj_digests, n);
  encode_u64_list(e, shard_digests, m);
  return std::move(e.buf);
}

std::string encode_patch_start_token(uint64_t token) {
  return encode_upsert_start(token);  // both are one u64
}

Result<uint64_t> decode_patch_start_token(const std::string& body) {
  serde::Dec d(body.data(), body.size());
  const uint64_t token = d.num<uint64_t>();
  if (!d.ok() || d.remaining() != 0) return bad("bad patch start request");
  return token;
}

std::string encode_patch_start_token_response(const PatchStartDigests& r) {
  serde::Enc e;
  encode_u64_list(e, r.obj_digests.data(), r.obj_digests.size());
  encode_u64_list(e, r.shard_digests.data(), r.shard_digests.size());
  return std::move(e.buf);
}

Result<PatchStartDigests> decode_patch_start_token_response(
    const std::string& body) {
  serde::Dec d(body.data(), body.size());
  PatchStartDigests r;
  if (!decode_u64_list(d, r.obj_digests) ||
      !decode_u64_list(d, r.shard_digests) || d.remaining() != 0)
    return bad("bad patch start response");
  return r;
}

Result<SessionOpen> decode_session_open(const std::string& body) {
  serde::Dec d(body.data(), body.size());
  SessionOpen r;
  const uint32_t count = d.num<uint32_t>();
  if (!count_fits(count, d)) return bad("bad session open request");
  r.keys.resize(count);
  r.sizes.resize(count);
  for (uint32_t i = 0; i < count && d.ok(); ++i) {
    r.keys[i] = d.str();
    r.sizes[i] = d.num<uint64_t>();
  }
  r.flags = d.num<uint8_t>();
  if (!d.ok() || d.remaining() != 0) return bad("bad session open request");
  return r;
}

Result<uint64_t> decode_session_open_response(const std::string& body) {
  serde::Dec d(body.data(), body.size());
  const uint64_t token = d.num<uint64_t>();
  if (!d.ok()) return bad("bad session open response");
  return token;
}

Result<CommitTokenShards> decode_commit_token_shards(const std::string& body) {
  serde::Dec d(body.data(), body.size());
  CommitTokenShards c;
  c.token = d.num<uint64_t>();
  c.flags = d.num<uint8_t>();
  if (!decode_u64_list(d, c.obj_digests) ||
      !decode_u64_list(d, c.shard_digests) || d.remaining() != 0)
    return bad("bad shard commit request");
  return c;
}

void append_item(BatchPlacements& out, PoolTable& table, int32_t status,
                 const std::vector<CopyPlacement>& copies, uint64_t size,
                 uint64_t checksum) {
  ItemPlaces it;
  it.status = status;
  it.size = size;
  it.checksum = checksum;
  it.first_place = static_cast<uint32_t>(out.places.size());
  for (auto& c : copies)
    for (size_t s = 0; s < c.shards.size(); ++s) {
      const uint16_t pi = table.intern(c.shards[s].pool_id);
      if (status == 0 && s == 0) {
        out.places.push_back({pi, c.shards[s].offset});
        ++it.ncopies;
      }
    }
  out.items.push_back(it);
}

std::string encode_put_start2_response(const BatchPlacements& p) {
  serde::Enc e;
  e.num<uint64_t>(p.view_version);
  e.num<uint64_t>(p.token);
  encode_pools(e, p.pools);
  encode_items(e, p, /*get=*/false);
  return std::move(e.buf);
}

std::string encode_get_workers2_response(const BatchPlacements& p) {
  serde::Enc e;
  encode_pools(e, p.pools);
  encode_items(e, p, /*get=*/true);
  return std::move(e.buf);
}

Result<void> decode_put_start2_response(const std::string& body, size_t nitems,
                                        BatchPlacements& out) {
  serde::Dec d(body.data(), body.size());
  out.view_version = d.num<uint64_t>();
  out.token = d.num<uint64_t>();
  return decode_response(d, nitems, /*get=*/false, out);
}

Result<void> decode_get_workers2_response(const std::string& body,
                                          size_t nitems, BatchPlacements& out) {
  serde::Dec d(body.data(), body.size());
  out.view_version = out.token = 0;
  return decode_response(d, nitems, /*get=*/true, out);
}

}  // namespace blackbird::wire
