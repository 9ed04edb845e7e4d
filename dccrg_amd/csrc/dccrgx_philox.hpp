// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy
// as 1, 2, 3", SC11), the counter-based generator of dccrgx_particles_create:
// ten rounds, the key bumped between them, no state.  Host and device.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define DX_HD __host__ __device__ __forceinline__
#else
#define DX_HD inline
#endif

namespace dccrgx {

DX_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
	for (int r = 0; r < 10; r++) {
		const uint64_t p0 = uint64_t(0xD2511F53u) * c0;
		const uint64_t p1 = uint64_t(0xCD9E8D57u) * c2;
		const uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0;
		const uint32_t n2 = uint32_t(p0 >> 32) ^ c3 ^ k1;
		c1 = uint32_t(p1);
		c3 = uint32_t(p0);
		c0 = n0;
		c2 = n2;
		k0 += 0x9E3779B9u;
		k1 += 0xBB67AE85u;
	}
	w[0] = c0;
	w[1] = c1;
	w[2] = c2;
	w[3] = c3;
}

// the uniform in [0, 1) of two output words: 53 bits, hi the upper 32
DX_HD double philox_uniform(uint32_t hi, uint32_t lo) {
	return double((uint64_t(hi) << 21) | uint64_t(lo >> 11)) * 0x1p-53;
}

}  // namespace dccrgx
