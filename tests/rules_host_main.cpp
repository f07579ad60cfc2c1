// Runs the engine's host rule preparation (csrc/pii_rules_host.h: blob parsing, derived tables, the packed
// rules buffer, the kernels' LDS images) on one blob file, without HIP.  Built with the host compiler and
// the address / undefined-behaviour sanitizers by tests/test_rules_host.py.
//
//   rules_host_main BLOB   prints "ok ..." or "rejected: <message>", exit status 0 either way; only a
//                          sanitizer report (or an unreadable file) gives another status
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "../context-based-pii_amd/csrc/pii_rules_host.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) return 2;
    const std::vector<uint8_t> blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    HostRules H;
    if (const char* why = build_host_rules(blob.data(), blob.size(), RuleKnobs{}, H)) {
        std::printf("rejected: %s\n", why);
        return 0;
    }
    const HostImage* ims[] = {&H.img_first, &H.img_first_hot, &H.img_eval, &H.img_eval_rg, &H.img_sel, &H.img_sel_rg,
                              &H.img_wsel};
    size_t img = 0;
    for (const HostImage* i : ims) img += i->bytes.size();
    std::printf("ok types=%d patterns=%d groups=%zu rules_bytes=%zu image_bytes=%zu\n", H.R.T, H.R.P,
                1 + H.groups.size(), H.packed.size(), img);
    return 0;
}
