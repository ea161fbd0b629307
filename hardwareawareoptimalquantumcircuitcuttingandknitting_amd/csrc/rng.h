// rng.h — the counter-based uniform stream of the samplers (qknit_sample.hip, qknit_shots.hip),
// mirrored on the host by oracle/sampling.py `uniforms`.
#ifndef QKNIT_RNG_H
#define QKNIT_RNG_H

#include <hip/hip_runtime.h>

#include <cstdint>

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// uniform double in [0, 1) for draw s of label l
__host__ __device__ __forceinline__ double draw(uint64_t seed, int64_t l, int64_t s) {
    const uint64_t z = splitmix64(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(l + 1) +
                                  0xD1B54A32D192ED03ull * (uint64_t)(s + 1));
    return (double)(z >> 11) * 0x1.0p-53;
}

#endif  // QKNIT_RNG_H
