// TEST INFRASTRUCTURE (CPU only, no GPU call): the host-side staging of ecfft_seq_min_poly / ecfft_seq_nth_term
// (ecfft_amd/csrc/seq_host.h): the bit length of the little-endian index and the size arithmetic that must not wrap.  Built with
// -fsanitize=address,undefined by tests/test_seq_host.py; every index lives in a heap buffer of exactly its length, so a read
// past either end is an error of the run.
// build: g++ -O1 -std=c++17 seq_host.cpp
#include "../../ecfft_amd/csrc/seq_host.h"
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
using namespace ecfft;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// the definition: the position of the highest set bit + 1
static size_t bits_slow(const std::vector<uint8_t>& e) {
    for (size_t i = 8 * e.size(); i-- > 0;)
        if ((e[i >> 3] >> (i & 7)) & 1) return i + 1;
    return 0;
}

int main() {
    size_t nbits = 99;
    CHECK(seq_index_bits(nullptr, 0, &nbits) && nbits == 0);
    std::mt19937_64 rng(7);
    for (size_t len = 1; len <= 40; ++len) {
        for (int rep = 0; rep < 200; ++rep) {
            std::vector<uint8_t> e(len);                          // exactly len bytes on the heap
            const int kind = rep % 4;
            for (auto& b : e) b = kind == 0 ? 0 : (uint8_t)rng();
            const size_t zeros = kind == 2 ? rng() % (len + 1) : 0;      // high zero bytes, up to all of them
            for (size_t i = 0; i < zeros; ++i) e[len - 1 - i] = 0;
            if (kind == 3) e[len - 1] = (uint8_t)(1u << (rng() % 8));    // one bit in the top byte
            nbits = 99;
            CHECK(seq_index_bits(e.data(), len, &nbits));
            CHECK(nbits == bits_slow(e));
            if (nbits) CHECK((e[(nbits - 1) >> 3] >> ((nbits - 1) & 7)) & 1);
        }
    }
    std::printf("index bit lengths: 8000 buffers of 1 .. 40 bytes\n");

    // products
    size_t x = 0;
    CHECK(seq_mul_fits(0, SIZE_MAX, &x) && x == 0);
    CHECK(seq_mul_fits(SIZE_MAX, 1, &x) && x == SIZE_MAX);
    CHECK(!seq_mul_fits(SIZE_MAX, 2, &x));
    CHECK(!seq_mul_fits((size_t)1 << 32, (size_t)1 << 32, &x));
    CHECK(seq_mul_fits((size_t)1 << 31, (size_t)1 << 32, &x) && x == (size_t)1 << 63);

    // the calls' shapes: what fits is exactly what fits in 128-bit arithmetic
    const size_t sizes[] = {0, 1, 2, 3, 255, 256, 4096, (size_t)1 << 20, (size_t)1 << 31, (size_t)1 << 40, (size_t)1 << 52, SIZE_MAX / 64, SIZE_MAX / 2, SIZE_MAX};
    for (size_t eb : {(size_t)4, (size_t)32})
        for (size_t n : sizes)
            for (size_t count : sizes)
                for (size_t leaves : {(size_t)1, (size_t)1024, (size_t)1 << 30}) {
                    const bool got = seq_min_poly_fits(n, count, leaves, eb);
                    bool want = n != 0 && count != 0 && n <= SIZE_MAX / (64 * eb) / 4;
                    if (want) {
                        const unsigned __int128 per = leaves > 4 * (n + 1) ? leaves : 4 * (n + 1);
                        want = per * 16 * eb * count <= (unsigned __int128)SIZE_MAX;
                    }
                    CHECK(got == want);
                    for (size_t nout : {(size_t)0, (size_t)1, (size_t)5, SIZE_MAX / 8}) {
                        const bool g2 = seq_nth_term_fits(n, nout, count, leaves, eb);
                        bool w2 = n >= 2 && nout != 0 && count != 0 && n <= SIZE_MAX / (64 * eb) && nout <= SIZE_MAX / (64 * eb);
                        if (w2) {
                            unsigned __int128 per = leaves > 2 * n ? leaves : 2 * n;
                            if (per < nout) per = nout;
                            w2 = per * 16 * eb * count <= (unsigned __int128)SIZE_MAX;
                        }
                        CHECK(g2 == w2);
                    }
                }
    std::printf("size arithmetic: every shape agrees with 128-bit arithmetic\n");
    if (fails) return 1;
    std::printf("SEQ_HOST_OK\n");
    return 0;
}
