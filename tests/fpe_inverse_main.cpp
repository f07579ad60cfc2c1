// Runs the decrypt form of the engine's FF1 body (csrc/pii_fpe.h: ff1_apply<true>, the very text k_reid
// compiles) on the CPU, without HIP.  Built with the host compiler and the address / undefined-behaviour
// sanitizers by tests/test_fpe_inverse_body.py; the sibling of fpe_body_main.cpp.
//
//   fpe_inverse_main FILE   FILE holds lines "<key record hex> <alphabet record hex> <surrogate hex> <finding hex>":
//                           the records as the compiler writes them (XF_FPE_KEY_WORDS and XF_FPE_ALPHA_WORDS
//                           little-endian words), then two byte strings ("-" = none).  Prints per line, as hex,
//                           the surrogate decrypted, and the finding encrypted by this program and then decrypted.
//                           Exit status 0 unless a line is malformed or a sanitizer reports.
// The decrypt form is called as k_reid calls it, with in == o, on a heap block of exactly the string's length
// and a numerals block of exactly XF_FPE_NMAX bytes, so a byte read or written outside them is reported.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../context-based-pii_amd/csrc/pii_fpe.h"

static bool unhex(const std::string& s, std::vector<uint8_t>& out) {
    out.clear();
    if (s == "-") return true;
    if (s.size() % 2) return false;
    for (size_t i = 0; i < s.size(); i += 2) {
        unsigned v;
        if (std::sscanf(s.c_str() + i, "%2x", &v) != 1) return false;
        out.push_back((uint8_t)v);
    }
    return true;
}

static uint8_t* block_of(const std::vector<uint8_t>& b) {
    uint8_t* p = new uint8_t[b.size()];
    if (!b.empty()) std::memcpy(p, b.data(), b.size());
    return p;
}

static void print_hex(const uint8_t* p, size_t n, char end) {
    if (n == 0) std::printf("-");
    for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
    std::printf("%c", end);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    if (!f) return 2;
    std::vector<uint32_t> te0(XF_FPE_TE0_WORDS);
    pii::fpe_te0(te0.data());
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        std::string hk, ha, hs, hf;
        std::vector<uint8_t> kb, ab, sb, fb;
        if (!(is >> hk >> ha >> hs >> hf) || !unhex(hk, kb) || !unhex(ha, ab) || !unhex(hs, sb) || !unhex(hf, fb)) return 3;
        if (kb.size() != 4 * XF_FPE_KEY_WORDS || ab.size() != 4 * XF_FPE_ALPHA_WORDS) return 3;
        std::vector<uint32_t> key(XF_FPE_KEY_WORDS), alpha(XF_FPE_ALPHA_WORDS);
        std::memcpy(key.data(), kb.data(), kb.size());
        std::memcpy(alpha.data(), ab.data(), ab.size());
        uint8_t* num = new uint8_t[XF_FPE_NMAX];
        // the surrogate, decrypted in place
        uint8_t* s = block_of(sb);
        std::memset(num, 0xAB, XF_FPE_NMAX);
        pii::ff1_apply<true>(te0.data(), key.data(), alpha.data(), s, (int)sb.size(), s, num, 1);
        print_hex(s, sb.size(), ' ');
        // the finding, encrypted as k_fpe does (a copy of it in the output), then decrypted in place
        uint8_t* in = block_of(fb);
        uint8_t* out = block_of(fb);
        std::memset(num, 0xAB, XF_FPE_NMAX);
        pii::ff1_apply(te0.data(), key.data(), alpha.data(), in, (int)fb.size(), out, num, 1);
        std::memset(num, 0xAB, XF_FPE_NMAX);
        pii::ff1_apply<true>(te0.data(), key.data(), alpha.data(), out, (int)fb.size(), out, num, 1);
        print_hex(out, fb.size(), '\n');
        delete[] s;
        delete[] in;
        delete[] out;
        delete[] num;
    }
    return 0;
}
