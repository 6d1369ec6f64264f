// The work-stealing fan-out the clients' batch paths and the keystone's
// maintenance passes share.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <future>
#include <vector>

namespace blackbird {

// Runs body(t, next) on max(1, min(threads, n)) spawned threads, t being the
// thread's number; next(i) hands each index of [0, n) out once across all of
// them and returns false when none is left. Never runs inline: a batch's
// transfers always execute on spawned threads.
template <typename Body>
void fan_out_threads(size_t n, int threads, Body&& body) {
  std::atomic<size_t> counter{0};
  auto next = [&](size_t& i) { return (i = counter.fetch_add(1)) < n; };
  const int nthreads =
      std::max(1, std::min<int>(threads, static_cast<int>(n)));
  std::vector<std::future<void>> futs;
  for (int t = 0; t < nthreads; ++t)
    futs.push_back(std::async(std::launch::async, [&, t] { body(t, next); }));
  for (auto& f : futs) f.get();
}

// fn(i) for every i in [0, n), spread over the threads above
template <typename Fn>
void fan_out(size_t n, int threads, Fn&& fn) {
  fan_out_threads(n, threads, [&](int, auto& next) {
    for (size_t i; next(i);) fn(i);
  });
}

}  // namespace blackbird
