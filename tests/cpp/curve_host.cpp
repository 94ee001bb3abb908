// Host instantiation of the curve search's Sylow computation (ecfft_amd/csrc/curve_search.h: the same __host__ __device__ steps the
// stage kernels run) on candidates 0 .. count-1 of a stream, for both fields.  Built with -fsanitize=address,undefined by
// tests/test_findcurve_host.py, which compares every printed line with the Python model (tests/curve_ref.py).  Also the CPU baseline:
// `curve_host <seed> <count> time` prints candidates per second on one core instead of the lines.
//
// build: g++ -O1 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include curve_host.cpp
// output: one line per candidate, "<field> <index> <n> <x as a standard-form hexadecimal integer>", then CURVE_HOST_OK
#include "../../ecfft_amd/csrc/curve_search.h"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace ecfft;

static void print_hex(uint32_t v) { printf("%x", v); }
static void print_hex(const Fe256& v) {
    int top = 7;
    while (top > 0 && v.l[top] == 0) --top;
    printf("%x", v.l[top]);
    for (int i = top - 1; i >= 0; --i) printf("%08x", v.l[i]);
}

template <class F>
static int run(const char* name, uint64_t seed, uint64_t count, bool timing) {
    using E = typename F::elem;
    const E half = F::inv(F::from_u32(2));
    if (!F::eq(F::add(half, half), F::one())) { printf("FAIL %s: 1/2\n", name); return 1; }
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t sum = 0;
    for (uint64_t i = 0; i < count; ++i) {
        const E a = curve::stream_elem<F>(seed, 8 * i), bb = curve::stream_elem<F>(seed, 8 * i + 4);
        E x;
        const uint32_t n = curve::sylow_host<F>(a, bb, half, &x);
        sum += n;
        if (timing) continue;
        // the chain of sqrt_canon against the bit-by-bit host square root
        E r0, r1 = F::sqrt_canon(bb);
        if (F::sqrt(bb, &r0) && !F::eq(r0, r1)) { printf("FAIL %s %llu: sqrt_canon\n", name, (unsigned long long)i); return 1; }
        if (n && !curve::is_square<F>(curve::rhs<F>(x, a, bb), &r0)) { printf("FAIL %s %llu: x is on no point\n", name, (unsigned long long)i); return 1; }
        printf("%s %llu %u ", name, (unsigned long long)i, n);
        print_hex(x);
        printf("\n");
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (timing) printf("%s candidates_per_s %.1f sum_n %llu\n", name, count / s, (unsigned long long)sum);
    return 0;
}

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 0) : 1, count = argc > 2 ? strtoull(argv[2], nullptr, 0) : 4096;
    const bool timing = argc > 3 && !strcmp(argv[3], "time");
    if (run<M31>("m31", seed, count, timing) || run<Secp256k1>("secp256k1", seed, count, timing)) return 1;
    printf("CURVE_HOST_OK\n");
    return 0;
}
