// bbctl — object store CLI: put/get/rm/exists/stat/workers/pools.
// Parity: reference clients/ucx_client.cpp (end-to-end demo CLI) as a real
// administration tool.
#include <fstream>
#include <iostream>
#include <sstream>

#include "blackbird/client/client.h"
#include "blackbird/rpc/methods.h"

using namespace blackbird;

static void usage() {
  std::cout <<
      "bbctl [--keystone H:P] <command> ...\n"
      "  put <key> <file|->      store a file (or stdin)\n"
      "  get <key> [file]        fetch an object (stdout by default)\n"
      "      --range OFF:LEN     only these bytes (unverified)\n"
      "  patch <key> <off> <file|->   overwrite bytes of an object in place\n"
      "      --edge-tiles        any range in place: tiles patched in part are\n"
      "                          composed of old and new bytes; the object is\n"
      "                          not re-verified (default: such a range rewrites\n"
      "                          and verifies the whole object)\n"
      "  rm <key>                remove an object\n"
      "  exists <key>\n"
      "  stat                    cluster stats\n"
      "  workers                 list workers\n"
      "  pools                   list memory pools\n"
      "  ls [prefix]             list objects\n"
      "  scrub [N] / repair / compact <pool>   maintenance\n"
      "  verify <key>            fetch + digest check\n"
      "options: --replication N --stripe N --class RAM_GPU|RAM_CPU|...\n";
}

int main(int argc, char** argv) {
  ClientOptions opts;
  PlacementConfig pcfg;
  std::vector<std::string> args;
  bool ranged = false;
  uint64_t range_off = 0, range_len = 0;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() -> std::string { return i + 1 < argc ? argv[++i] : ""; };
    if (a == "--keystone") opts.keystone_endpoint = next();
    else if (a == "--replication") pcfg.replication = atoi(next().c_str());
    else if (a == "--stripe") pcfg.max_workers_per_copy = atoi(next().c_str());
    else if (a == "--range") {
      const std::string r = next();
      const auto colon = r.find(':');
      if (colon == std::string::npos || colon == 0 || colon + 1 == r.size()) {
        std::cerr << "--range wants OFF:LEN\n";
        return 1;
      }
      ranged = true;
      range_off = strtoull(r.substr(0, colon).c_str(), nullptr, 0);
      range_len = strtoull(r.substr(colon + 1).c_str(), nullptr, 0);
    } else if (a == "--edge-tiles") {
      opts.patch_edge_tiles = true;
    } else if (a == "--class") {
      auto c = storage_class_from_string(next());
      if (c) pcfg.preferred_class = *c;
    } else if (a == "--help" || a == "-h") {
      usage();
      return 0;
    } else args.push_back(a);
  }
  if (args.empty()) {
    usage();
    return 1;
  }

  Client client(opts);
  if (auto r = client.connect(); !r.ok()) {
    std::cerr << "connect failed: " << r.message() << "\n";
    return 1;
  }

  const std::string& cmd = args[0];
  auto fail = [](const char* what, const auto& r) {
    std::cerr << what << " failed: " << to_string(r.code()) << " " << r.message()
              << "\n";
    return 1;
  };

  // a file's bytes, or stdin's for "-"
  auto slurp = [](const std::string& path, std::string& data) {
    std::ostringstream ss;
    if (path == "-") {
      ss << std::cin.rdbuf();
    } else {
      std::ifstream in(path, std::ios::binary);
      if (!in) {
        std::cerr << "cannot open " << path << "\n";
        return false;
      }
      ss << in.rdbuf();
    }
    data = ss.str();
    return true;
  };

  if (cmd == "put" && args.size() >= 3) {
    std::string data;
    if (!slurp(args[2], data)) return 1;
    auto r = client.put(args[1], data.data(), data.size(), pcfg);
    if (!r.ok()) return fail("put", r);
    std::cout << "stored " << args[1] << " (" << data.size() << " bytes)\n";
  } else if (cmd == "patch" && args.size() >= 4) {
    std::string data;
    if (!slurp(args[3], data)) return 1;
    const uint64_t off = strtoull(args[2].c_str(), nullptr, 0);
    auto r = client.patch(args[1], off, data.data(), data.size());
    if (!r.ok()) return fail("patch", r);
    std::cout << "patched " << args[1] << " (" << data.size() << " bytes at "
              << off << ")\n";
  } else if (cmd == "get" && args.size() >= 2) {
    auto r = ranged ? client.get_range(args[1], range_off, range_len)
                    : client.get(args[1]);
    if (!r.ok()) return fail("get", r);
    if (args.size() >= 3) {
      std::ofstream out(args[2], std::ios::binary);
      out.write(r.value().data(), static_cast<std::streamsize>(r.value().size()));
      std::cout << "wrote " << r.value().size() << " bytes to " << args[2] << "\n";
    } else {
      std::cout.write(r.value().data(), static_cast<std::streamsize>(r.value().size()));
    }
  } else if (cmd == "rm" && args.size() >= 2) {
    auto r = client.remove(args[1]);
    if (!r.ok()) return fail("rm", r);
    std::cout << "removed " << args[1] << "\n";
  } else if (cmd == "exists" && args.size() >= 2) {
    auto r = client.exists(args[1]);
    if (!r.ok()) return fail("exists", r);
    std::cout << (r.value() ? "yes" : "no") << "\n";
    return r.value() ? 0 : 2;
  } else if (cmd == "verify" && args.size() >= 2) {
    ClientOptions vo = opts;
    vo.verify_checksum_on_get = true;
    Client vc(vo);
    if (auto r = vc.connect(); !r.ok()) return fail("connect", r);
    auto r = vc.get(args[1]);
    if (!r.ok()) return fail("verify", r);
    std::cout << "ok (" << r.value().size() << " bytes, digest verified)\n";
  } else if (cmd == "stat") {
    auto r = client.cluster_stats();
    if (!r.ok()) return fail("stat", r);
    auto& s = r.value();
    std::cout << "workers=" << s.num_workers << " pools=" << s.num_pools
              << " objects=" << s.num_objects << " used=" << s.total_used << "/"
              << s.total_capacity << " view=" << s.view_version << "\n";
  } else if (cmd == "workers") {
    auto r = client.workers_info();
    if (!r.ok()) return fail("workers", r);
    for (auto& w : r.value())
      std::cout << w.worker_id << "\t" << w.node_id << "\t" << w.data_endpoint
                << "\n";
  } else if (cmd == "pools") {
    auto r = client.memory_pools();
    if (!r.ok()) return fail("pools", r);
    for (auto& p : r.value())
      std::cout << p.pool_id << "\t" << p.worker_id << "\t"
                << to_string(p.storage_class) << "\t" << p.used << "/" << p.size
                << "\n";
  } else if (cmd == "ls") {
    auto r = client.list_objects(args.size() >= 2 ? args[1] : "", 10000);
    if (!r.ok()) return fail("ls", r);
    for (auto& o : r.value())
      std::cout << o.key << "\t" << o.size << "\t" << o.ncopies << "x\t"
                << to_string(o.storage_class) << "\n";
  } else if (cmd == "scrub") {
    blackbird::serde::Enc e;
    e.num<uint32_t>(args.size() >= 2 ? atoi(args[1].c_str()) : 0);
    auto r = client.meta_call_raw(blackbird::rpc::methods::ADMIN_SCRUB, e.buf);
    if (!r.ok()) return fail("scrub", r);
    blackbird::serde::Dec d(r.value().data(), r.value().size());
    std::cout << "quarantined " << d.num<uint64_t>() << " corrupt copies\n";
  } else if (cmd == "repair") {
    auto r = client.meta_call_raw(blackbird::rpc::methods::ADMIN_REPAIR, {});
    if (!r.ok()) return fail("repair", r);
    std::cout << "repair pass done\n";
  } else if (cmd == "compact" && args.size() >= 2) {
    blackbird::serde::Enc e;
    e.str(args[1]);
    auto r = client.meta_call_raw(blackbird::rpc::methods::ADMIN_COMPACT, e.buf);
    if (!r.ok()) return fail("compact", r);
    blackbird::serde::Dec d(r.value().data(), r.value().size());
    std::cout << "moved " << d.num<uint64_t>() << " objects\n";
  } else {
    usage();
    return 1;
  }
  return 0;
}
