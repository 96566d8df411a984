// rex_philox.h -- Philox4x32-10 and the task draw of a REX_TASK_MIXED batch, one text for the kernels (rex_kernels.h) and for the
// host code that places the envs of such a batch into waves (rex_placement.h).  rex_gym_amd/envs/philox.py is the independent
// reference the tests compare against.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define REX_HD __host__ __device__ __forceinline__
#else
#define REX_HD inline
#endif

namespace rex {

// high half of a 32 x 32 bit product (the device keeps its own instruction next to the separate low multiply)
REX_HD uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// ---- Philox4x32-10 ----
REX_HD void philox4x32(uint32_t* c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = philox_mulhi(0xD2511F53u, c[0]), l0 = 0xD2511F53u * c[0];
    const uint32_t h1 = philox_mulhi(0xCD9E8D57u, c[2]), l1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = h1 ^ c[1] ^ k0, n1 = l1, n2 = h0 ^ c[3] ^ k1, n3 = l0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// The slot (index into the mix, < n_mix) of the task env `gidx` runs for its whole life in a REX_TASK_MIXED batch: a draw from its
// own Philox stream, block 2 of episode 0xFFFFFFFF -- behind env_reset (0) and env_ground (1), in front of the sensor noise (16 ...).
REX_HD int mixed_task_draw(uint32_t seed_lo, uint32_t seed_hi, int gidx, int n_mix) {
  uint32_t ctr[4] = {0xFFFFFFFFu, (uint32_t)gidx, 2u, 0u};
  philox4x32(ctr, seed_lo, seed_hi);
  return (int)(ctr[0] % (uint32_t)n_mix);
}

}  // namespace rex
