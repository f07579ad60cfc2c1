// Runs the engine's host rule preparation (csrc/pii_rules_host.h: blob parsing, derived tables, the packed
// rules buffer, the kernels' LDS images) on one blob file, without HIP.  Built with the host compiler and
// the address / undefined-behaviour sanitizers by tests/rules_host_runner.py.
//
//   rules_host_main BLOB   prints "ok ... digest=<hex>" or "rejected: <message>", exit status 0 either
//                          way; only a sanitizer report (or an unreadable file) gives another status.
//                          The digest (64-bit FNV-1a) covers everything the preparation produced.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../context-based-pii_amd/csrc/pii_rules_host.h"

struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void* p, size_t n) {
        for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const uint8_t*>(p)[i]) * 0x100000001b3ull;
    }
    void num(uint64_t v) { bytes(&v, 8); }
    template <class V>
    void vec(const V& v) {   // (the length first: two vectors never run together)
        num(v.size());
        if (!v.empty()) bytes(v.data(), v.size() * sizeof(v[0]));
    }
};

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
                              &H.img_wsel, &H.img_xtext};
    size_t img = 0;
    for (const HostImage* i : ims)
        if (i != &H.img_xtext) img += i->bytes.size();
    Fnv d;
    const RulesDev& R = H.R;
    for (int64_t v : {(int64_t)R.P, (int64_t)R.G, (int64_t)R.T, (int64_t)R.V, (int64_t)R.SD, (int64_t)R.CD,
                      (int64_t)R.d_start, (int64_t)R.SK, (int64_t)R.CK, (int64_t)R.k_start, (int64_t)R.n_hot,
                      (int64_t)R.min_len, (int64_t)R.kw_always_min, (int64_t)R.NE, (int64_t)R.CDs, (int64_t)R.CKs,
                      (int64_t)R.dsh, (int64_t)R.n_dacc, (int64_t)R.n_kacc, (int64_t)R.nl_off})
        d.num((uint64_t)v);
    d.vec(H.packed);
    for (size_t o : H.off) d.num(o);
    d.num(H.groups.size());
    for (const HostGroup& g : H.groups) {
        for (int64_t v : {(int64_t)g.SD, (int64_t)g.CD, (int64_t)g.CDs, (int64_t)g.dsh, (int64_t)g.lds}) d.num((uint64_t)v);
        for (size_t o : g.off) d.num(o);
    }
    d.num(H.scan_lds);
    for (const HostImage* i : ims) {
        for (uint32_t o : i->li.off) d.num(o);
        d.num(i->li.total);
        d.num(i->li.aux);
        d.num(i->global);
        d.vec(i->bytes);
    }
    d.num(H.first_p_hot);
    for (bool b : {H.lists_cl, H.xf_src, H.xf_mask, H.xf_hash, H.window_ok, H.excl_general, H.excl_lists, H.excl_text})
        d.num(b);
    d.num((uint64_t)H.excl_nx);
    d.vec(H.xf_kind);
    d.num(H.names.size());
    for (const std::string& s : H.names) d.vec(s);
    d.vec(H.kw_type);
    std::printf("ok types=%d patterns=%d groups=%zu rules_bytes=%zu image_bytes=%zu digest=%016llx\n", H.R.T, H.R.P,
                1 + H.groups.size(), H.packed.size(), img, (unsigned long long)d.h);
    return 0;
}
