// Host instantiation of the short-Weierstrass front end for both fields: build_short_weierstrass and check_short_weierstrass
// (ecfft_amd/csrc/host_curve.h: what ecfft_build_ec_fftree runs before any device work) and the group law the point kernels run
// (ecfft_amd/csrc/curve_points.h, __host__ __device__).  Built with -fsanitize=address,undefined by tests/test_ectree_host.py,
// which writes the commands and compares every printed line with the Python model (tests/ec_ref.py).
//
// build: g++ -O1 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include ec_tree_host.cpp
// usage: ec_tree_host <command file>; one command per line, integers in decimal, fields m31 / secp256k1:
//   tree  <field> <A> <B> <gen x> <gen y> <log order> <off x> <off y> <log n>
//       -> "tree <rc>", then per level "map <num0> <num1> <num2> <den0> <den1> <den2>", then "leaf <x>" per leaf, then per inner
//          layer "layer <k> <x> ..." (all standard-form hexadecimal)
//   check <field> <A> <B> <gen x> <gen y> <log order> <off x> <off y>       -> "check <0|1>"
//   mul   <field> <A> <B> <x> <y> <scalar, hexadecimal>                     -> "mul <x> <y>" or "mul inf", and "adic <two-adicity of the result>"
// The last line is EC_TREE_HOST_OK.
#include "../../ecfft_amd/csrc/host_curve.h"
#include "../../ecfft_amd/csrc/curve_points.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

using namespace ecfft;

static void print_hex(uint32_t v) { printf("%x", v); }
static void print_hex(const Fe256& v) {
    int top = 7;
    while (top > 0 && v.l[top] == 0) --top;
    printf("%x", v.l[top]);
    for (int i = top - 1; i >= 0; --i) printf("%08x", v.l[i]);
}
template <class F> typename F::elem parse(const std::string& s);
template <> uint32_t parse<M31>(const std::string& s) { return (uint32_t)(strtoull(s.c_str(), nullptr, 10) % M31::P); }
template <> Fe256 parse<Secp256k1>(const std::string& s) { return Secp256k1::from_dec(s.c_str()); }

template <class F>
static int run(const std::string& cmd, std::istringstream& in) {
    using E = typename F::elem;
    auto elem = [&]() { std::string s; in >> s; return parse<F>(s); };
    const E A = elem(), B = elem();
    if (cmd == "mul") {
        const E x = elem(), y = elem();
        std::string hex; in >> hex;
        uint8_t k[ecpoint::kMaxScalarBytes] = {0};
        if (hex.size() > 2 * sizeof(k)) return 1;
        for (size_t i = 0; i < hex.size(); ++i) {                   // the last digit is the lowest nibble
            const char c = hex[hex.size() - 1 - i];
            const unsigned d = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
            k[i / 2] |= (uint8_t)(d << (4 * (i & 1)));
        }
        const unsigned nbits = ecpoint::scalar_bits(k, 1, sizeof(k));
        const ecpoint::Jac<F> r = ecpoint::jac_mul<F>(x, y, k, sizeof(k), nbits, A);
        E ox, oy;
        if (ecpoint::jac_to_affine<F>(r, &ox, &oy)) { printf("mul "); print_hex(ox); printf(" "); print_hex(oy); printf("\n"); }
        else printf("mul inf\n");
        printf("adic %d\n", ecpoint::jac_two_adicity<F>(r, kMaxTwoAdicity<F>, A));
        return 0;
    }
    Pt<F> gen, off;
    gen.x = elem(); gen.y = elem(); gen.inf = false;
    unsigned log_order = 0, log_n = 0;
    in >> log_order;
    off.x = elem(); off.y = elem(); off.inf = false;
    if (cmd == "check") { printf("check %d\n", check_short_weierstrass<F>(A, B, gen, log_order, off) ? 1 : 0); return 0; }
    if (cmd != "tree") return 1;
    in >> log_n;
    HostTree<F> t;
    const int rc = build_short_weierstrass<F>(A, B, gen, log_order, off, log_n, t, /*points=*/true);
    printf("tree %d\n", rc);
    if (rc) return 0;
    for (const RatMap<F>& m : t.maps) {
        printf("map");
        for (int i = 0; i < 3; ++i) { printf(" "); print_hex(m.num[i]); }
        for (int i = 0; i < 3; ++i) { printf(" "); print_hex(m.den[i]); }
        printf("\n");
    }
    for (size_t i = 0; i < t.n; ++i) { printf("leaf "); print_hex(t.f[t.n + i]); printf("\n"); }
    unsigned k = 1;
    for (size_t sz = t.n / 2; sz >= 1; sz >>= 1, ++k) {
        printf("layer %u", k);
        for (size_t i = 0; i < sz; ++i) { printf(" "); print_hex(t.f[sz + i]); }
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: ec_tree_host <command file>\n"); return 2; }
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string cmd, field;
        if (!(in >> cmd >> field)) continue;
        const int rc = field == "m31" ? run<M31>(cmd, in) : (field == "secp256k1" ? run<Secp256k1>(cmd, in) : 1);
        if (rc) { printf("FAIL %s\n", line.c_str()); return 1; }
    }
    printf("EC_TREE_HOST_OK\n");
    return 0;
}
