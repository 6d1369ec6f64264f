// Exact CPU reference of the bbhash64 object digest (see
// csrc/include/blackbird/gpu/digest_spec.h). Used to verify the MFMA kernel
// bit-for-bit and to checksum DRAM/disk-tier objects — so it is also
// optimized: AVX2 madd inner product (~20× over the scalar loop) and a
// thread fan-out for large objects (the digest is a commutative u64 sum, so
// any tile partition is bit-exact).
#include <cstring>
#include <future>
#include <thread>
#include <vector>

#if defined(__AVX2__)
#include <immintrin.h>
#endif

#include "blackbird/gpu/digest_spec.h"

namespace blackbird::gpu {

using namespace blackbird::digest;

namespace {

struct Tables {
  int8_t B[32][32];
  uint32_t W[1024];
#if defined(__AVX2__)
  // interleaved B for _mm256_madd_epi16: for k-pair kp and column block cb
  // (8 cols), lanes = [B[2kp][c], B[2kp+1][c]] per column, widened to i16.
  alignas(32) int16_t Bi[16][4][16];  // [kpair][colblock][16 i16 lanes]
#endif
  Tables() {
    for (int k = 0; k < 32; ++k)
      for (int c = 0; c < 32; ++c) B[k][c] = b_matrix(k, c);
    for (int i = 0; i < 1024; ++i) W[i] = w_weight(i);
#if defined(__AVX2__)
    for (int kp = 0; kp < 16; ++kp)
      for (int cb = 0; cb < 4; ++cb)
        for (int c = 0; c < 8; ++c) {
          Bi[kp][cb][2 * c] = B[2 * kp][cb * 8 + c];
          Bi[kp][cb][2 * c + 1] = B[2 * kp + 1][cb * 8 + c];
        }
#endif
  }
};

const Tables& tables() {
  static Tables t;
  return t;
}

// Digest contribution of tiles [t0, t1) of `p` (`nbytes` valid bytes at
// `p`); slot indices are offset by `slot_base` tiles (streaming chunks).
uint64_t hash_tiles(const uint8_t* p, uint64_t nbytes, uint64_t t0, uint64_t t1,
                    uint64_t slot_base = 0) {
  const Tables& tb = tables();
  uint64_t H = 0;
  int32_t C[32][32];
  int8_t A[32][32];

  for (uint64_t t = t0; t < t1; ++t) {
    const uint64_t base = t * kTileBytes;
    const uint64_t avail = nbytes > base ? nbytes - base : 0;
    const int8_t* a;
    if (avail >= kTileBytes) {
      a = reinterpret_cast<const int8_t*>(p + base);
    } else {
      std::memset(A, 0, sizeof(A));
      std::memcpy(A, p + base, avail);
      a = &A[0][0];
    }

#if defined(__AVX2__)
    for (int r = 0; r < 32; ++r) {
      __m256i acc0 = _mm256_setzero_si256();
      __m256i acc1 = _mm256_setzero_si256();
      __m256i acc2 = _mm256_setzero_si256();
      __m256i acc3 = _mm256_setzero_si256();
      const int8_t* ar = a + r * 32;
      for (int kp = 0; kp < 16; ++kp) {
        // broadcast the (A[r][2kp], A[r][2kp+1]) i16 pair to all lanes
        const int32_t pair =
            (static_cast<uint16_t>(static_cast<int16_t>(ar[2 * kp]))) |
            (static_cast<int32_t>(static_cast<int16_t>(ar[2 * kp + 1])) << 16);
        const __m256i av = _mm256_set1_epi32(pair);
        acc0 = _mm256_add_epi32(
            acc0, _mm256_madd_epi16(
                      av, _mm256_load_si256(
                              reinterpret_cast<const __m256i*>(tb.Bi[kp][0]))));
        acc1 = _mm256_add_epi32(
            acc1, _mm256_madd_epi16(
                      av, _mm256_load_si256(
                              reinterpret_cast<const __m256i*>(tb.Bi[kp][1]))));
        acc2 = _mm256_add_epi32(
            acc2, _mm256_madd_epi16(
                      av, _mm256_load_si256(
                              reinterpret_cast<const __m256i*>(tb.Bi[kp][2]))));
        acc3 = _mm256_add_epi32(
            acc3, _mm256_madd_epi16(
                      av, _mm256_load_si256(
                              reinterpret_cast<const __m256i*>(tb.Bi[kp][3]))));
      }
      _mm256_storeu_si256(reinterpret_cast<__m256i*>(&C[r][0]), acc0);
      _mm256_storeu_si256(reinterpret_cast<__m256i*>(&C[r][8]), acc1);
      _mm256_storeu_si256(reinterpret_cast<__m256i*>(&C[r][16]), acc2);
      _mm256_storeu_si256(reinterpret_cast<__m256i*>(&C[r][24]), acc3);
    }
#else
    for (int r = 0; r < 32; ++r)
      for (int c = 0; c < 32; ++c) {
        int32_t acc = 0;
        for (int k = 0; k < 32; ++k)
          acc += static_cast<int32_t>(a[r * 32 + k]) *
                 static_cast<int32_t>(tb.B[k][c]);
        C[r][c] = acc;
      }
#endif

    for (int g = 0; g < 64; ++g) {
      uint64_t f = 0;
      const int col = fold_col(g);
      for (int j = 0; j < 16; ++j) {
        const int row = fold_row(g, j);
        f += static_cast<uint64_t>(static_cast<uint32_t>(C[row][col])) *
             static_cast<uint64_t>(tb.W[row * 32 + col]);
      }
      H += mix64(f + tile_weight((slot_base + t) * 64 + g));
    }
  }
  return H;
}

}  // namespace

uint64_t checksum_cpu_tiles(const void* chunk, uint64_t nbytes,
                            uint64_t first_tile) {
  const uint64_t ntiles = (nbytes + kTileBytes - 1) / kTileBytes;
  return hash_tiles(static_cast<const uint8_t*>(chunk), nbytes, 0, ntiles,
                    first_tile);
}

uint64_t checksum_cpu_finalize(uint64_t h, uint64_t object_nbytes) {
  return finalize(h, object_nbytes);
}

uint64_t checksum_cpu_unfinalize(uint64_t digest, uint64_t object_nbytes) {
  return unfinalize(digest, object_nbytes);
}

uint64_t checksum_cpu(const void* ptr, uint64_t nbytes) {
  const uint8_t* p = static_cast<const uint8_t*>(ptr);
  const uint64_t ntiles = (nbytes + kTileBytes - 1) / kTileBytes;

  uint64_t H = 0;
  const uint64_t kParallelThreshold = 512;  // tiles (512 KiB)
  if (ntiles >= kParallelThreshold) {
    unsigned nthreads = std::min(8u, std::thread::hardware_concurrency());
    if (nthreads < 2) nthreads = 2;
    const uint64_t per = (ntiles + nthreads - 1) / nthreads;
    std::vector<std::future<uint64_t>> futs;
    for (unsigned i = 0; i < nthreads; ++i) {
      uint64_t t0 = i * per;
      uint64_t t1 = std::min(ntiles, t0 + per);
      if (t0 >= t1) break;
      futs.push_back(std::async(std::launch::async, [=] {
        return hash_tiles(p, nbytes, t0, t1);
      }));
    }
    for (auto& f : futs) H += f.get();
  } else {
    H = hash_tiles(p, nbytes, 0, ntiles);
  }
  return finalize(H, nbytes);
}

}  // namespace blackbird::gpu
