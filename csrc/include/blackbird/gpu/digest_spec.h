// Specification of the Blackbird-MI355X object digest ("bbhash64").
// Shared by the CDNA4 MFMA kernel (csrc/hip/digest.hip) and the exact CPU
// reference (csrc/common/checksum_cpu.cpp) — all math is wraparound u64/u32
// and fully commutative, so GPU and CPU produce identical bits regardless of
// execution order.
//
// Definition:
//   data is consumed in 1024-B tiles; tile t is the row-major 32×32 int8
//   matrix A_t (A[r][k] = (int8)byte[t*1024 + r*32 + k], zero-padded tail).
//   C_t = A_t × B  (int32, wraparound), B the fixed pseudo-random 32×32 int8
//   matrix below.
//
//   The 1024 elements of C_t are partitioned into 64 fold groups of 16 —
//   group g owns elements {(row(g,j), col(g)) : j ∈ [0,16)} with
//     col(g)    = g & 31
//     row(g,j)  = (j & 3) + 8*(j >> 2) + 4*(g >> 5)
//   (this fixed partition matches the CDNA4 mfma_i32_32x32x* accumulator
//   lane mapping, so the GPU folds AGPRs in place with no cross-lane step —
//   but it is defined here purely arithmetically and the CPU reproduces it).
//
//   Group fold:  f(t,g) = Σ_j (u64)( (u32)C[row][col] * W[row*32+col] )
//                         (32×32→64 full multiply, u64 wraparound sum)
//   Digest:      H = Σ_{t,g} mix64( f(t,g) + tile_weight(t*64 + g) )
//   finalized as mix64(H ^ nbytes).  Empty object: finalize(0, 0).
//
// This is a corruption-detection checksum (random dense linear code over the
// bytes, position-weighted, avalanche-mixed), not a cryptographic hash: any
// single flipped bit perturbs 32 weighted C elements; collisions of
// independent corruptions occur w.p. ≈ 2^-64.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define BB_HD __host__ __device__
#else
#define BB_HD
#endif

namespace blackbird::digest {

constexpr uint64_t kTileBytes = 1024;

BB_HD constexpr uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

BB_HD constexpr uint64_t mix64(uint64_t x) {
  x = (x ^ (x >> 33)) * 0xFF51AFD7ED558CCDull;
  x = (x ^ (x >> 33)) * 0xC4CEB9FE1A85EC53ull;
  return x ^ (x >> 33);
}

// Positional weight for (tile, fold-group) slot s = t*64 + g.
BB_HD constexpr uint64_t tile_weight(uint64_t s) {
  return splitmix64(s ^ 0xB1ACB19D00000001ull);
}

// Fixed projection matrix B[k][c], k,c ∈ [0,32).
BB_HD constexpr int8_t b_matrix(int k, int c) {
  return static_cast<int8_t>(splitmix64(0xB000ull + k * 32 + c) & 0xFF);
}

// Per-element fold weight W[pos], pos = r*32+c ∈ [0,1024).
BB_HD constexpr uint32_t w_weight(int pos) {
  return static_cast<uint32_t>(splitmix64(0xF01Dull + pos) & 0xFFFFFFFFull);
}

BB_HD constexpr int fold_col(int g) { return g & 31; }
BB_HD constexpr int fold_row(int g, int j) {
  return (j & 3) + 8 * (j >> 2) + 4 * (g >> 5);
}

BB_HD constexpr uint64_t finalize(uint64_t h, uint64_t nbytes) {
  return mix64(h ^ nbytes);
}

// mix64 is a bijection of u64 (xorshifts by >= 32 are involutions, the
// multipliers are odd), so a recorded digest gives its sum H back: what an
// in-place patch adds its tiles' term differences to (patch_plan.h).
constexpr uint64_t kUnmixMul1 = 0x9CB4B2F8129337DBull;  // 0xC4CEB9FE1A85EC53^-1
constexpr uint64_t kUnmixMul2 = 0x4F74430C22A54005ull;  // 0xFF51AFD7ED558CCD^-1
static_assert(kUnmixMul1 * 0xC4CEB9FE1A85EC53ull == 1);
static_assert(kUnmixMul2 * 0xFF51AFD7ED558CCDull == 1);

BB_HD constexpr uint64_t unmix64(uint64_t x) {
  x = (x ^ (x >> 33)) * kUnmixMul1;
  x = (x ^ (x >> 33)) * kUnmixMul2;
  return x ^ (x >> 33);
}

BB_HD constexpr uint64_t unfinalize(uint64_t digest, uint64_t nbytes) {
  return unmix64(digest) ^ nbytes;
}

static_assert(unmix64(mix64(0x0123456789ABCDEFull)) == 0x0123456789ABCDEFull);
static_assert(mix64(unmix64(~0ull)) == ~0ull);
static_assert(unfinalize(finalize(0xB1ACB19Dull, 3849), 3849) == 0xB1ACB19Dull);

}  // namespace blackbird::digest
