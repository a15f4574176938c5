// GPU probe (gfx950): accumulation of v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3 operands.  D = A B with all
// rows of A equal, so every value of lane l is dot(a, B[:, l & 31]) (operand layout: fp8_mfma_probe.hip); each
// is compared on the host with the exact dot product (64 products of <= 8 significant bits: exact in double).
// Measured on MI355X: 54530 of 65536 dot products differ from the correctly rounded fp32 sum, by up to
// 3376 x 2^-23 x max |product| (most by 2^8 .. 2^10 x 2^-23 x max |product|): the instruction does not return
// the correctly rounded sum, which is why tests/tower_faithful.py cannot track an 8-bit tower bit for bit.
// build: hipcc --offload-arch=gfx950 -O2 -o build/fp8_acc_probe tools/probes/fp8_mfma_accumulation_probe.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
static double e4m3_to_double(uint8_t b) {
	const int e = (b >> 3) & 15, m = b & 7;
	double v = e == 0 ? std::ldexp(double(m), -9) : std::ldexp(1.0 + m / 8.0, e - 7);
	return (b & 0x80) ? -v : v;
}
__global__ void k(const uint8_t *A, const uint8_t *B, float *D, int n) {
	const int t = blockIdx.x, lane = threadIdx.x;
	if (t >= n) return;
	v8i a, b;
	for (int i = 0; i < 8; ++i) {
		a[i] = reinterpret_cast<const int *>(A + (size_t)t * 64 * 32)[lane * 8 + i];
		b[i] = reinterpret_cast<const int *>(B + (size_t)t * 64 * 32)[lane * 8 + i];
	}
	f32x16 c = {};
	c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);
	for (int i = 0; i < 16; ++i) D[((size_t)t * 64 + lane) * 16 + i] = c[i];
}
int main() {
	const int n = 2048;
	std::mt19937 rng(11);
	std::vector<uint8_t> A((size_t)n * 2048), B((size_t)n * 2048);
	auto rnd = [&](int emin, int emax) {
		for (;;) {
			int e = emin + int(rng() % unsigned(emax - emin + 1)), m = int(rng() % 8);
			uint8_t b = uint8_t((rng() & 1) << 7 | (e << 3) | m);
			if ((b & 0x7f) != 0x7f) return b;
		}
	};
	std::vector<double> av(64), bv(64 * 32);
	for (int t = 0; t < n; ++t) {
		int emax = 4 + t % 12;  // exponent fields 0 .. emax: wide and narrow ranges
		uint8_t arow[64];
		for (int kk = 0; kk < 64; ++kk) arow[kk] = rnd(0, emax);
		for (int l = 0; l < 64; ++l) {
			const int h = l >> 5;
			for (int j = 0; j < 32; ++j) {
				A[(size_t)t * 2048 + l * 32 + j] = arow[32 * h + j];
				B[(size_t)t * 2048 + l * 32 + j] = rnd(0, emax);
			}
		}
	}
	uint8_t *dA, *dB; float *dD;
	hipMalloc(&dA, A.size()); hipMalloc(&dB, B.size()); hipMalloc(&dD, (size_t)n * 64 * 16 * 4);
	hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice);
	hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice);
	hipLaunchKernelGGL(k, dim3(n), dim3(64), 0, 0, dA, dB, dD, n);
	if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
	std::vector<float> D((size_t)n * 64 * 16);
	hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost);
	// histogram of |err| / (max |product| * 2^-23), and share not equal to the fp32-rounded exact sum
	long neq = 0, tot = 0, incons = 0;
	double worst = 0, worstRelSum = 0;
	int hist[40] = {0};
	for (int t = 0; t < n; ++t) {
		for (int l = 0; l < 32; ++l) {
			double exact = 0, pmax = 0;
			for (int kk = 0; kk < 64; ++kk) {
				const int h = kk >> 5, j = kk & 31;
				const double p = e4m3_to_double(A[(size_t)t * 2048 + (h * 32 + l) * 32 + j]) *
				                 e4m3_to_double(B[(size_t)t * 2048 + (h * 32 + l) * 32 + j]);
				exact += p;  // exact: products have <= 8 significant bits in [2^-18, 2^17.6]
				pmax = std::fmax(pmax, std::fabs(p));
			}
			const float g = D[((size_t)t * 64 + l) * 16];
			for (int i = 1; i < 16; ++i) if (D[((size_t)t * 64 + l) * 16 + i] != g) ++incons;
			++tot;
			if (g != float(exact)) ++neq;
			const double u = std::fabs(g - exact) / (pmax * std::ldexp(1.0, -23));
			worst = std::fmax(worst, u);
			int bin = u == 0 ? 0 : std::min(39, 1 + std::max(0, int(std::floor(std::log2(u))) + 20));
			hist[bin]++;
			worstRelSum = std::fmax(worstRelSum, std::fabs(g - exact) / std::fmax(std::fabs(exact), 1e-30));
		}
	}
	printf("dots %ld, not equal to fp32(exact) %ld, inconsistent lanes %ld\n", tot, neq, incons);
	printf("worst |err| / (max|p| 2^-23) = %.4g, worst rel to |exact| = %.4g\n", worst, worstRelSum);
	printf("hist (bin 0: exact-zero err; bin b: u in [2^(b-21), 2^(b-20))):");
	for (int b = 0; b < 40; ++b) if (hist[b]) printf(" %d:%d", b, hist[b]);
	printf("\n");
	// the first few mismatches
	int shown = 0;
	for (int t = 0; t < n && shown < 6; ++t) {
		for (int l = 0; l < 32 && shown < 6; ++l) {
			double exact = 0, pmax = 0;
			for (int kk = 0; kk < 64; ++kk) {
				const int h = kk >> 5, j = kk & 31;
				const double p = e4m3_to_double(A[(size_t)t * 2048 + (h * 32 + l) * 32 + j]) *
				                 e4m3_to_double(B[(size_t)t * 2048 + (h * 32 + l) * 32 + j]);
				exact += p; pmax = std::fmax(pmax, std::fabs(p));
			}
			const float g = D[((size_t)t * 64 + l) * 16];
			if (g != float(exact)) { printf("t %d col %d exact %.17g fp32 %.9g got %.9g pmax %.6g\n", t, l, exact, float(exact), g, pmax); ++shown; }
		}
	}
	return 0;
}
