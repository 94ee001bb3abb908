// Host-side staging of ecfft_seq_min_poly / ecfft_seq_nth_term: the bit length of the index and the size arithmetic that must not
// wrap.  Plain C++, no device call: tests/cpp/seq_host.cpp drives it under AddressSanitizer and UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ecfft {

// The number of significant bits of the little-endian integer e[0 .. bytes): high zero bytes do not count, 0 for the value 0 (e
// may then be null).  False where the bit count would not fit the kernels' uint32_t.
inline bool seq_index_bits(const uint8_t* e, size_t bytes, size_t* nbits) {
    while (bytes && e[bytes - 1] == 0) --bytes;
    *nbits = 0;
    if (bytes == 0) return true;
    if (bytes > UINT32_MAX / 8) return false;
    size_t n = 8 * bytes;
    while (!((e[(n - 1) >> 3] >> ((n - 1) & 7)) & 1)) --n;
    *nbits = n;
    return true;
}
// a * b, or false where it wraps
inline bool seq_mul_fits(size_t a, size_t b, size_t* out) {
    if (a && b > SIZE_MAX / a) return false;
    *out = a * b;
    return true;
}
// ecfft_seq_min_poly: the byte counts of the rows (count x n, count x (n / 2 + 1)) and of the temporaries of a row of the large
// regime (16 rows of max(leaves, 4 (n + 1)) elements, the bound of ecfft_poly_xgcd_partial) must not wrap
inline bool seq_min_poly_fits(size_t n, size_t count, size_t leaves, size_t elem_bytes) {
    if (n == 0 || count == 0 || n > SIZE_MAX / (64 * elem_bytes) / 4) return false;
    const size_t per = leaves > 4 * (n + 1) ? leaves : 4 * (n + 1);
    size_t x;
    return seq_mul_fits(per, 16 * elem_bytes, &x) && seq_mul_fits(x, count, &x);
}
// ecfft_seq_nth_term: count x (nc + L + nout) elements of rows and 16 count max(leaves, 2 nc) of temporaries must not wrap
inline bool seq_nth_term_fits(size_t nc, size_t nout, size_t count, size_t leaves, size_t elem_bytes) {
    if (nc < 2 || nout == 0 || count == 0 || nc > SIZE_MAX / (64 * elem_bytes) || nout > SIZE_MAX / (64 * elem_bytes)) return false;
    size_t per = leaves > 2 * nc ? leaves : 2 * nc;
    if (per < nout) per = nout;
    size_t x;
    return seq_mul_fits(per, 16 * elem_bytes, &x) && seq_mul_fits(x, count, &x);
}

}  // namespace ecfft
