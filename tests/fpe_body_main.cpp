// Runs the engine's FF1 body (csrc/pii_fpe.h: ff1_apply, the very text k_fpe and k_win_fpe compile) on the
// CPU, without HIP.  Built with the host compiler and the address / undefined-behaviour sanitizers by
// tests/test_fpe_body.py.
//
//   fpe_body_main FILE   FILE holds lines "<key record hex> <alphabet record hex> <finding hex>": a key
//                        record of XF_FPE_KEY_WORDS and an alphabet record of XF_FPE_ALPHA_WORDS little-endian
//                        words, as the compiler writes them, and the finding's bytes ("-" = none).  Prints the
//                        transformed finding as hex per line ("-" = none).  Exit status 0 unless a line is
//                        malformed or a sanitizer reports.
// The finding and the output are heap blocks of exactly the finding's length and the numerals one of
// exactly XF_FPE_NMAX bytes, so a byte read or written outside them is reported.
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

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    if (!f) return 2;
    std::vector<uint32_t> te0(XF_FPE_TE0_WORDS);
    pii::fpe_te0(te0.data());
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        std::string hk, ha, hf;
        std::vector<uint8_t> kb, ab, fb;
        if (!(is >> hk >> ha >> hf) || !unhex(hk, kb) || !unhex(ha, ab) || !unhex(hf, fb)) return 3;
        if (kb.size() != 4 * XF_FPE_KEY_WORDS || ab.size() != 4 * XF_FPE_ALPHA_WORDS) return 3;
        std::vector<uint32_t> key(XF_FPE_KEY_WORDS), alpha(XF_FPE_ALPHA_WORDS);
        std::memcpy(key.data(), kb.data(), kb.size());
        std::memcpy(alpha.data(), ab.data(), ab.size());
        uint8_t* in = new uint8_t[fb.size()];
        uint8_t* out = new uint8_t[fb.size()];
        uint8_t* num = new uint8_t[XF_FPE_NMAX];
        if (!fb.empty()) std::memcpy(in, fb.data(), fb.size());
        if (!fb.empty()) std::memcpy(out, fb.data(), fb.size());      // (as k_redact<true> leaves it)
        std::memset(num, 0xAB, XF_FPE_NMAX);
        pii::ff1_apply(te0.data(), key.data(), alpha.data(), in, (int)fb.size(), out, num, 1);
        if (fb.empty()) std::printf("-");
        for (size_t i = 0; i < fb.size(); ++i) std::printf("%02x", out[i]);
        std::printf("\n");
        delete[] in;
        delete[] out;
        delete[] num;
    }
    return 0;
}
