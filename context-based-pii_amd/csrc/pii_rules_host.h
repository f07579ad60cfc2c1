// pii_rules_host.h - everything pii_engine_create does before its first HIP call: blob parsing, the
// derived host tables, the packed rules buffer, the kernels' LDS images.  Plain C++17 (no HIP header),
// so a host compiler alone builds and runs it (tests/rules_host_main.cpp, under the sanitizers).
//
// build_host_rules(blob, knobs) -> a HostRules value, or the message of the first defect it met.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pii_engine.h"
#include "pii_layout.h"

namespace {

// ------------------------------------------------------------------------------- blob parsing
struct Section {
    std::string name;
    uint32_t dtype;
    const uint8_t* data;
    uint64_t bytes;
    std::vector<uint64_t> own;    // an 8-byte aligned copy, when the blob's bytes are not (see parse_blob)
};

// A section's data follows its name, so the blob places it at any byte offset, while the tables are read
// as u16 / u32 / i64 arrays: a section that is not 8-byte aligned in memory is copied.
inline bool parse_blob(const uint8_t* p, size_t n, std::vector<Section>& out) {
    if (n < 12 || std::memcmp(p, "PIIRULE1", 8) != 0) return false;
    uint32_t cnt;
    std::memcpy(&cnt, p + 8, 4);
    size_t off = 12;
    for (uint32_t i = 0; i < cnt; ++i) {
        uint32_t ln;
        if (off + 4 > n) return false;
        std::memcpy(&ln, p + off, 4);
        off += 4;
        if (off + ln + 12 > n) return false;
        Section s;
        s.name.assign(reinterpret_cast<const char*>(p + off), ln);
        off += ln;
        std::memcpy(&s.dtype, p + off, 4);
        std::memcpy(&s.bytes, p + off + 4, 8);
        off += 12;
        if (s.bytes > n || off + s.bytes > n) return false;
        s.data = p + off;
        off += s.bytes;
        off += (8 - off % 8) % 8;
        out.push_back(std::move(s));
    }
    for (Section& s : out)
        if (reinterpret_cast<uintptr_t>(s.data) % 8 != 0) {
            s.own.assign((s.bytes + 7) / 8 + 1, 0);
            std::memcpy(s.own.data(), s.data, s.bytes);
            s.data = reinterpret_cast<const uint8_t*>(s.own.data());
        }
    return true;
}

// ------------------------------------------------------------------------------- LDS images
// DFAs re-packed into a kernel's own pool (descriptor offsets rebased; each transition entry carries
// the destination's flags in bits 14-15, see pii_device.h)
struct DfaPool {
    std::vector<uint16_t> trans;
    std::vector<uint8_t> cmap;
    std::vector<int32_t> desc;
};
// pre: a FIRST automaton's PRE state (absorbed match starts, first_begin), -1 = none
inline bool add_dfa(DfaPool& dp, const int32_t* d, const uint16_t* trans, const uint8_t* flags, const uint8_t* cmap,
                    int32_t pre = -1) {
    const int32_t nc = d[3], ns = d[7];
    if (ns > (int32_t)pii::DFA_STATE_MASK + 1) return false;
    int32_t nd[8];
    std::memcpy(nd, d, sizeof(nd));
    // LDS bank stagger (32 banks x 4 B): a pair kernel's wavefront runs many patterns' automata over
    // the same text bytes, so automaton k's transition table starts at bank k mod 32 and its class map
    // 4 bytes after the previous map's end (byte c of every map would otherwise sit in one bank)
    const size_t k = dp.desc.size() / 8;
    while (dp.trans.size() % 64 != (2 * k) % 64) dp.trans.push_back(0);
    nd[0] = (int32_t)dp.trans.size();
    nd[1] = pre < 0 ? 0 : pre + 1;
    nd[2] = (int32_t)dp.cmap.size();
    for (size_t i = 0; i < (size_t)ns * nc; ++i) {
        const uint16_t dst = trans[d[0] + i];
        dp.trans.push_back((uint16_t)(dst | ((flags[d[1] + dst] & 3u) << 14)));
    }
    dp.cmap.insert(dp.cmap.end(), cmap + d[2], cmap + d[2] + 256);
    dp.cmap.insert(dp.cmap.end(), 4, (uint8_t)0);
    dp.desc.insert(dp.desc.end(), nd, nd + 8);
    return true;
}

// a per-(variant, type) list table, deduplicated for the LDS images (list_range)
struct ListTab {
    std::vector<uint8_t> ix;      // per key: list number, w bytes
    std::vector<uint32_t> loff;   // per list: first id, + end
    std::vector<uint16_t> ids;
    uint32_t w = 1;
};
// (a small table stays as it is -- w = 0, ix empty: one LDS read less per lookup; config 2's list
// lookups in k_select cost 4 us more through the index)
constexpr size_t LIST_DEDUP_KEYS = 8192;
inline ListTab dedup_lists(const uint32_t* off, const uint16_t* ids, size_t n_keys) {
    ListTab t;
    if (n_keys <= LIST_DEDUP_KEYS) {
        t.w = 0;
        t.ix.push_back(0);
        t.loff.assign(off, off + n_keys + 1);
        t.ids.assign(ids, ids + off[n_keys]);
        if (t.ids.empty()) t.ids.push_back(0);
        return t;
    }
    std::map<std::vector<uint16_t>, uint32_t> uniq;
    std::vector<uint32_t> num(n_keys);
    t.loff.push_back(0);
    for (size_t i = 0; i < n_keys; ++i) {
        std::vector<uint16_t> l(ids + off[i], ids + off[i + 1]);
        auto it = uniq.find(l);
        if (it == uniq.end()) {
            it = uniq.emplace(l, (uint32_t)uniq.size()).first;
            t.ids.insert(t.ids.end(), l.begin(), l.end());
            t.loff.push_back((uint32_t)t.ids.size());
        }
        num[i] = it->second;
    }
    const size_t n = uniq.size();
    t.w = n <= 256 ? 1u : (n <= 65536 ? 2u : 4u);
    t.ix.resize(n_keys * t.w);
    for (size_t i = 0; i < n_keys; ++i) std::memcpy(t.ix.data() + i * t.w, &num[i], t.w);   // little endian
    if (t.ids.empty()) t.ids.push_back(0);
    return t;
}

// one kernel's image on the host: its bytes and section offsets; empty = not built
struct HostImage {
    LdsImage li{};
    std::vector<uint8_t> bytes;
    bool global = false;      // larger than LDS: kernels read it in place (load_image<true>)
};
using ImageParts = std::vector<std::pair<const void*, size_t>>;
template <class V>
std::pair<const void*, size_t> part(const V& v) {
    return {(const void*)v.data(), v.size() * sizeof(v[0])};
}
// packs `parts` (16-byte aligned sections) into one image
inline bool pack_image(const ImageParts& parts, uint32_t aux, HostImage& out) {
    if (parts.size() > (size_t)IMG_MAX) return false;
    size_t off = 0;
    for (size_t i = 0; i < parts.size(); ++i) {
        out.li.off[i] = (uint32_t)off;
        off += (parts[i].second + 15) & ~(size_t)15;
    }
    if (off == 0) off = 16;
    out.li.total = (uint32_t)off;
    out.li.aux = aux;
    out.global = off > IMG_LDS_MAX;
    out.bytes.assign(off, 0);
    for (size_t i = 0; i < parts.size(); ++i)
        if (parts[i].second) std::memcpy(out.bytes.data() + out.li.off[i], parts[i].first, parts[i].second);
    return true;
}

// ------------------------------------------------------------------------------- host rules
// the tables of the packed rules buffer, in the order they are placed (256-byte aligned sections); the
// SCAN groups' tables follow TB_XF_MASK, the hash tables come after every other table (rules without a
// hash type keep their layout), the general exclusion tables after those (likewise); the text exclusion
// rules live in their kernel's image alone
enum { TB_CMAP4, TB_TD, TB_TK, TB_D_ACCID, TB_D_ACC_OFF, TB_D_ACC_IDS, TB_K_ACCID, TB_K_ACC_MIN, TB_D_NPAIR, TB_K_GRP,
       TB_D_NA, TB_DET_TYPE, TB_DET_VAL, TB_DET_LIK, TB_DET_EXIDX, TB_FIRST_DESC, TB_HOT_RULE, TB_HOT_DESC,
       TB_VAR_ENABLED, TB_VAR_MINLIK, TB_RULE_OFF, TB_RULE_IDS, TB_EXCL_OFF, TB_EXCL_IDS, TB_TOK_OFF, TB_TOK_BYTES,
       TB_TOK_LEN, TB_XF_KIND, TB_XF_MASK, TB_HASH_KEY, TB_HASH_MID, TB_XG_OFF, TB_XG_IDS, TB_XG_IDX, TB_N };
enum { GT_CMAP4, GT_TD, GT_TK, GT_D_ACCID, GT_K_ACCID, GT_D_NPAIR, GT_N };

// a SCAN group >= 1: its own D automaton and class map, a 1-row never-accepting K stub
struct HostGroup {
    int SD, CD, CDs, dsh;        // (its start row is row 0)
    uint32_t lds;
    size_t off[GT_N];
};

// the PII_* environment knobs that shape the images (the engine's other knobs: EngineKnobs)
struct RuleKnobs {
    bool first_drop = true;                 // PII_FIRST_DROP=0: no absorbed match starts
    size_t first_hot_big = FIRST_HOT_BIG;   // PII_FIRST_HOT_BIG
    size_t first_hot_lds = FIRST_HOT_LDS;   // PII_FIRST_HOT_LDS
    uint32_t first_hot = 0xffffffffu;       // PII_FIRST_HOT: at most this many patterns in the hot FIRST copy
};

struct HostRules {
    RulesDev R{};                      // the scalar fields; the table pointers are set after the upload
    std::vector<uint8_t> packed;       // every table of the rules buffer
    size_t off[TB_N] = {};
    std::vector<HostGroup> groups;
    size_t scan_lds = 0;
    HostImage img_first, img_first_hot, img_eval, img_eval_rg, img_sel, img_sel_rg, img_wsel;
    HostImage img_xtext;               // k_excl_text's (text exclusion rules only)
    uint32_t first_p_hot = 0;
    bool lists_cl = false;
    std::vector<std::string> names;
    std::vector<int> kw_type;
    std::vector<uint8_t> xf_kind;
    bool xf_src = false, xf_mask = false, xf_hash = false;
    bool window_ok = false;
    // general exclusion rules (var.xg_off / var.xg_ids / det.xgidx): k_exclude decides them, the
    // streaming lists are empty; excl_nx = its excluder patterns
    bool excl_general = false;
    int excl_nx = 0;
    bool excl_lists = false;           // some (variant, type) has an exclude_info_types list: k_exclude's phases run
    // text exclusion rules (var.xt_off / var.xt_ids / xt.*): k_excl_text decides them (img_xtext)
    bool excl_text = false;
};

// entry (row, class) = address of the destination row | accept | accept of the destination's
// end-of-text transition (class C-1) << 1, so k_scan resets at an utterance start without
// reading the end-of-text entry
// (k_scan: rows are placed with the START state first -- row = pos(state) -- and entries are the
// destination row's byte offset from the table base, so a reset is "row 0"; the class words carry
// the table bases; accept-id tables follow the same placement)
inline void relayout(const uint16_t* s, const uint16_t* acc, int S, int C, int Cs, int start, uint16_t* t, uint16_t* a,
                     int dsh = 0) {
    auto pos = [start](uint32_t r) { return r == (uint32_t)start ? 0u : r == 0 ? (uint32_t)start : r; };
    for (int r = 0; r < S; ++r)
        for (int c = 0; c < C; ++c) {
            const uint32_t v = s[r * C + c], dst = v & 0x7fff;
            const uint32_t eot = s[dst * C + C - 1] >> 15;
            t[pos(r) * Cs + c] = (uint16_t)(((pos(dst) * Cs * 2) >> dsh) | (v >> 15) | (eot << 1));
            a[pos(r) * Cs + c] = acc[r * C + c];
        }
}

// The FIRST automata of k_pair_first<true>'s LDS copy (an image past LDS): patterns in id order (the
// built-in types first), skipping any automaton over `big` bytes, until the copy is full.  A skipped
// pattern keeps a descriptor with no columns (read from L2).  Returns the patterns covered.
template <class Pre>
uint32_t pack_first_hot(const RuleKnobs& k, int P, const int32_t* fdesc, const uint16_t* ptrans, const uint8_t* pflags,
                        const uint8_t* pcmap, Pre fpre, DfaPool& hf) {
    const size_t big = k.first_hot_big, budget = k.first_hot_lds;
    const uint32_t cap_p = std::min<uint32_t>((uint32_t)P, k.first_hot);
    auto bytes_with = [&](size_t tr, size_t cm, size_t np) {
        return ((tr * 2 + 15) & ~(size_t)15) + ((cm + 260 + 15) & ~(size_t)15) + ((np * 32 + 15) & ~(size_t)15);
    };
    uint32_t ph = 0;
    size_t trans_n = 0, cmap_n = 0;
    for (uint32_t p = 0; p < cap_p; ++p) {
        const int32_t* d = fdesc + 8 * p;
        const size_t dfa = (size_t)d[7] * d[3] * 2, tr = trans_n + 64 + (size_t)d[7] * d[3];
        if (bytes_with(tr, cmap_n, p + 1) > budget) {
            if (big == 0) break;
            continue;
        }
        if (big && dfa > big) continue;
        trans_n = tr;
        cmap_n += 260;
        ph = p + 1;
    }
    for (uint32_t p = 0; p < ph; ++p) {
        const int32_t* d = fdesc + 8 * p;
        const size_t dfa = (size_t)d[7] * d[3] * 2, tr = hf.trans.size() + 64 + (size_t)d[7] * d[3];
        if ((big && dfa > big) || bytes_with(tr, hf.cmap.size(), ph) > budget) {
            hf.desc.insert(hf.desc.end(), 8, 0);          // columns 0: not resident
            continue;
        }
        add_dfa(hf, d, ptrans, pflags, pcmap, fpre((int)p));
    }
    return ph;
}

// Returns nullptr and fills `H`, or the first defect of the blob.
inline const char* build_host_rules(const uint8_t* blob, size_t n, const RuleKnobs& knobs, HostRules& H) {
    std::vector<Section> secs;
    if (!parse_blob(blob, n, secs)) return "not a rules blob";
    auto find = [&](const std::string& nm) -> const Section* {
        for (auto& s : secs)
            if (s.name == nm) return &s;
        return nullptr;
    };
    static const char* req[] = {"meta", "scan.cmap2", "scan.d.trans", "scan.d.accid", "scan.d.acc_off",
                                "scan.d.acc_ids", "scan.k.trans", "scan.k.accid", "scan.k.acc_off", "scan.k.acc_ids",
                                "det.type", "det.validator", "det.lik", "det.exidx", "det.first_desc", "hot.rule",
                                "hot.dfa_desc", "pool.trans", "pool.flags", "pool.cmap", "var.enabled",
                                "var.minlik", "var.rule_off", "var.rule_ids", "var.excl_off", "var.excl_ids",
                                "kw.type", "kw.always", "types.names"};
    for (auto r : req)
        if (!find(r)) return "a required section is missing";
    auto u16 = [&](const char* nm) { return reinterpret_cast<const uint16_t*>(find(nm)->data); };
    auto u32 = [&](const char* nm) { return reinterpret_cast<const uint32_t*>(find(nm)->data); };
    auto i32 = [&](const char* nm) { return reinterpret_cast<const int32_t*>(find(nm)->data); };
    const int64_t* meta = reinterpret_cast<const int64_t*>(find("meta")->data);
    RulesDev& R = H.R;
    int* const dims[] = {&R.P, &R.G, &R.T, &R.V, &R.SD, &R.CD, &R.d_start, &R.SK, &R.CK, &R.k_start, &R.n_hot, &R.min_len};
    for (int i = 0; i < 12; ++i) *dims[i] = (int)meta[i];
    R.min_len = (int)std::max<int64_t>(1, meta[11]);
    H.window_ok = meta[13] != 0;
    if (R.P > 65535) return "too many detector patterns";
    // scan table entries are 16-bit LDS byte addresses (k_scan layout: class map, D rows, K rows);
    // rows are padded to an even class count so every row address is a multiple of 4 and bit 1 of
    // an entry is free for the destination's end-of-text accept
    R.CDs = (R.CD + 1) & ~1;
    R.CKs = (R.CK + 1) & ~1;
    R.dsh = 0;
    const uint32_t td_words = (uint32_t)(R.SD * R.CDs / 2), tk_words = (uint32_t)(R.SK * R.CKs / 2);
    const uint32_t tk_base = SCAN_TD_BASE + td_words * 4;
    if ((uint64_t)tk_base + (uint64_t)tk_words * 4 > 65536) return "SCAN tables exceed 64 KiB of LDS";
    if (R.T > 65535) return "too many types";
    {   // names
        const Section* s = find("types.names");
        const char* p = reinterpret_cast<const char*>(s->data);
        for (size_t i = 0; i < s->bytes;) {
            const size_t l = strnlen(p + i, s->bytes - i);
            H.names.emplace_back(p + i, l);
            i += l + 1;
        }
        if ((int)H.names.size() != R.T) return "type table mismatch";
    }
    for (int g = 0; g < R.G; ++g) H.kw_type.push_back(u16("kw.type")[g]);
    // host-side derived tables
    std::vector<uint16_t> td(R.SD * R.CDs, 0), tk(R.SK * R.CKs, 0), dacc(R.SD * R.CDs, 0), kacc(R.SK * R.CKs, 0);
    relayout(u16("scan.d.trans"), u16("scan.d.accid"), R.SD, R.CD, R.CDs, R.d_start, td.data(), dacc.data());
    relayout(u16("scan.k.trans"), u16("scan.k.accid"), R.SK, R.CK, R.CKs, R.k_start, tk.data(), kacc.data());
    R.d_start = R.k_start = 0;                                     // row offsets: the start rows are first
    std::vector<uint32_t> cmap4(256);
    {
        const uint16_t* c2 = u16("scan.cmap2");
        for (int b = 0; b < 256; ++b)
            cmap4[b] = (SCAN_TD_BASE + 2u * (c2[b] & 0xffu)) | (tk_base + 2u * (uint32_t)(c2[b] >> 8)) << 16;
    }
    std::vector<uint16_t> k_acc_min;
    {
        const uint32_t* off = u32("scan.k.acc_off");
        const uint16_t* ids = u16("scan.k.acc_ids");
        const size_t nsets = find("scan.k.acc_off")->bytes / 4 - 1;
        R.n_kacc = (uint32_t)nsets;
        R.n_dacc = (uint32_t)(find("scan.d.acc_off")->bytes / 4 - 1);
        for (size_t a = 0; a < nsets; ++a) {
            int m = KW_NONE;
            for (uint32_t i = off[a]; i < off[a + 1]; ++i) m = std::min<int>(m, ids[i]);
            k_acc_min.push_back((uint16_t)m);
        }
    }
    R.kw_always_min = KW_NONE;
    for (int g = 0; g < R.G; ++g)
        if (find("kw.always")->data[g]) {
            R.kw_always_min = g;
            break;
        }
    {
        const uint8_t* ex = find("det.exidx")->data;
        int ne = 0;
        for (int p = 0; p < R.P; ++p)
            if (ex[p] != 0xff) ne = std::max(ne, ex[p] + 1);
        if (ne > NE_MAX) return "too many excluder patterns";
        R.NE = ne;
    }
    // general exclusion rules: the three sections together or not at all, beside empty streaming lists
    const Section *xs_goff = find("var.xg_off"), *xs_gids = find("var.xg_ids"), *xs_gidx = find("det.xgidx");
    if (xs_goff || xs_gids || xs_gidx) {
        if (!xs_goff || !xs_gids || !xs_gidx) return "general exclusion sections are not all present";
        if (R.V < 0 || R.T < 0 || R.P < 0) return "general exclusion tables malformed";
        const size_t keys = (size_t)R.V * R.T;
        if (xs_goff->bytes != (keys + 1) * 4) return "var.xg_off does not hold V*T+1 offsets";
        if (xs_gidx->bytes != (size_t)R.P) return "det.xgidx does not hold one index per pattern";
        const uint32_t* go = reinterpret_cast<const uint32_t*>(xs_goff->data);
        const uint16_t* gi = reinterpret_cast<const uint16_t*>(xs_gids->data);
        if (go[0] != 0) return "var.xg_off does not start at 0";
        for (size_t k = 0; k < keys; ++k)
            if (go[k] > go[k + 1]) return "var.xg_off is not ascending";
        if ((uint64_t)go[keys] * 2 > xs_gids->bytes) return "var.xg_ids is shorter than its offsets";
        for (uint32_t q = 0; q < go[keys]; ++q)
            if ((gi[q] & (XG_PARTIAL - 1)) >= R.T) return "var.xg_ids names a type past the type table";
        int nx = 0;
        for (int p = 0; p < R.P; ++p)
            if (xs_gidx->data[p] != 0xff) {
                if (xs_gidx->data[p] >= NX_MAX) return "det.xgidx holds an index past the limit";
                nx = std::max(nx, xs_gidx->data[p] + 1);
            }
        const Section* xo = find("var.excl_off");
        if (R.NE != 0 || xo->bytes < (keys + 1) * 4 || reinterpret_cast<const uint32_t*>(xo->data)[keys] != 0)
            return "general exclusion sections beside streaming exclusion lists";
        H.excl_general = true;
        H.excl_nx = nx;
        H.excl_lists = go[keys] != 0;
    }
    // text exclusion rules: the seven sections together or not at all, and only beside the general ones
    static const char* const xt_names[] = {"var.xt_off", "var.xt_ids", "xt.rule", "xt.desc", "xt.trans", "xt.flags",
                                           "xt.cmap"};
    const Section* xts[7];
    int xt_present = 0;
    for (int i = 0; i < 7; ++i) xt_present += (xts[i] = find(xt_names[i])) != nullptr;
    DfaPool xp;
    ListTab xtl;
    if (xt_present) {
        if (xt_present != 7) return "text exclusion sections are not all present";
        if (!H.excl_general) return "text exclusion sections without the general exclusion sections";
        const Section *s_off = xts[0], *s_ids = xts[1], *s_rule = xts[2], *s_desc = xts[3], *s_tr = xts[4], *s_fl = xts[5],
                      *s_cm = xts[6];
        const size_t keys = (size_t)R.V * R.T;
        const size_t nr = s_rule->bytes / 16;
        if (nr == 0 || s_rule->bytes % 16 != 0 || nr > 65535) return "xt.rule does not hold whole rules";
        if (s_desc->bytes != nr * 32) return "xt.desc does not hold one descriptor per rule";
        if (s_cm->bytes != nr * 256) return "xt.cmap does not hold one class map per rule";
        if (s_off->bytes != (keys + 1) * 4) return "var.xt_off does not hold V*T+1 offsets";
        const uint32_t* xo = reinterpret_cast<const uint32_t*>(s_off->data);
        const uint16_t* xi = reinterpret_cast<const uint16_t*>(s_ids->data);
        if (xo[0] != 0) return "var.xt_off does not start at 0";
        for (size_t k = 0; k < keys; ++k)
            if (xo[k] > xo[k + 1]) return "var.xt_off is not ascending";
        if ((uint64_t)xo[keys] * 2 > s_ids->bytes) return "var.xt_ids is shorter than its offsets";
        for (uint32_t q = 0; q < xo[keys]; ++q)
            if (xi[q] >= nr) return "var.xt_ids names a rule past the rule table";
        const int32_t* xr = reinterpret_cast<const int32_t*>(s_rule->data);
        const int32_t* xd = reinterpret_cast<const int32_t*>(s_desc->data);
        const uint16_t* xtr = reinterpret_cast<const uint16_t*>(s_tr->data);
        for (size_t r = 0; r < nr; ++r) {
            const int32_t kind = xr[4 * r], wb = xr[4 * r + 1], wa = xr[4 * r + 2];
            if (kind < 0 || kind >= XT_KINDS) return "xt.rule holds an unknown kind";
            if (wb < 0 || wa < 0) return "xt.rule holds a negative window";
            if (kind == XT_HOTWORD && wb == 0 && wa == 0) return "xt.rule holds a hotword rule without a window";
            const int32_t* d = xd + 8 * r;
            const int64_t nc = d[3], ns = d[7];
            if (nc < 2 || nc > 256 || ns < 1 || ns > (int64_t)pii::DFA_STATE_MASK + 1)
                return "xt.desc holds an automaton of impossible size";
            if (d[0] < 0 || (uint64_t)d[0] + (uint64_t)(ns * nc) > s_tr->bytes / 2)
                return "xt.desc points past xt.trans";
            if (d[1] < 0 || (uint64_t)d[1] + (uint64_t)ns > s_fl->bytes) return "xt.desc points past xt.flags";
            if (d[2] < 0 || (uint64_t)d[2] + 256 > s_cm->bytes) return "xt.desc points past xt.cmap";
            if (d[4] < 0 || d[4] >= ns) return "xt.desc holds a start state past its automaton";
            for (int64_t i = 0; i < ns * nc; ++i)
                if (xtr[d[0] + i] >= ns) return "xt.trans holds a state past its automaton";
            for (int c = 0; c < 256; ++c)
                if (s_cm->data[d[2] + c] >= nc - 1) return "xt.cmap holds a class past its automaton";
            if (!add_dfa(xp, d, xtr, s_fl->data, s_cm->data)) return "xt.desc holds an automaton of impossible size";
        }
        xtl = dedup_lists(xo, xi, keys);
        H.excl_text = true;
    }
    // deidentify_config: without the sections every type is replaced by its "[NAME]" token
    static const char* xf_bad = "transformation tables malformed";
    H.xf_kind.assign(R.T, (uint8_t)PII_XF_INFO_TYPE);
    std::vector<uint32_t> xf_maskp((size_t)std::max(R.T, 1) * XF_MASK_WORDS, 0u);
    const Section *xs_repl_off = nullptr, *xs_repl = nullptr, *xs_hkey = nullptr, *xs_hmid = nullptr;
    if (const Section* xk = find("xf.kind")) {
        xs_repl_off = find("xf.repl_off");
        xs_repl = find("xf.repl");
        const Section* xm = find("xf.mask");
        if (xk->bytes != (size_t)R.T || !xs_repl_off || !xs_repl || !xm || xs_repl_off->bytes != ((size_t)R.T + 1) * 4 ||
            xm->bytes != (size_t)R.T * XF_MASK_WORDS * 4)
            return xf_bad;
        const uint32_t* ro = reinterpret_cast<const uint32_t*>(xs_repl_off->data);
        for (int t = 0; t < R.T; ++t) {
            if (xk->data[t] > PII_XF_HASH || ro[t] > ro[t + 1] || ro[t + 1] > xs_repl->bytes || ro[t + 1] - ro[t] > 255)
                return xf_bad;
            H.xf_kind[t] = xk->data[t];
            H.xf_src |= xk->data[t] == PII_XF_MASK || xk->data[t] == PII_XF_KEEP;
            H.xf_mask |= xk->data[t] == PII_XF_MASK;
            H.xf_hash |= xk->data[t] == PII_XF_HASH;
        }
        if (H.xf_hash) {   // per type a key index, per key two midstates; a hash type's replacement is its placeholder
            xs_hkey = find("xf.hash_key");
            xs_hmid = find("xf.hash_mid");
            if (!xs_hkey || !xs_hmid || xs_hkey->bytes != (size_t)R.T * 4 || xs_hmid->bytes == 0 ||
                xs_hmid->bytes % (XF_HASH_KEY_WORDS * 4) != 0)
                return xf_bad;
            const uint32_t* hk = reinterpret_cast<const uint32_t*>(xs_hkey->data);
            for (int t = 0; t < R.T; ++t)
                if (H.xf_kind[t] == PII_XF_HASH &&
                    (hk[t] >= xs_hmid->bytes / (XF_HASH_KEY_WORDS * 4) || ro[t + 1] - ro[t] != XF_HASH_LEN))
                    return xf_bad;
        }
        std::memcpy(xf_maskp.data(), xm->data, xm->bytes);
        for (int t = 0; t < R.T; ++t)
            if (H.xf_kind[t] == PII_XF_MASK && (xf_maskp[(size_t)t * XF_MASK_WORDS] & 0xffu) > 127u) return xf_bad;
    }
    // tok_len: the per-type output length table behind out_len (T + 1 entries, as the offsets it replaces
    // in the k_select / k_win_select images)
    std::vector<uint32_t> tok_off(R.T + 1, 0), tok_len(R.T + 1, 0);
    std::string tok;
    for (int t = 0; t < R.T; ++t) {
        if (H.xf_kind[t] == PII_XF_INFO_TYPE) {
            tok += "[" + H.names[t] + "]";
        } else if (H.xf_kind[t] == PII_XF_REPLACE || H.xf_kind[t] == PII_XF_HASH) {   // (hash: the placeholder)
            const uint32_t* ro = reinterpret_cast<const uint32_t*>(xs_repl_off->data);
            tok.append(reinterpret_cast<const char*>(xs_repl->data) + ro[t], ro[t + 1] - ro[t]);
        }
        tok_off[t + 1] = (uint32_t)tok.size();
        const bool same_len = H.xf_kind[t] == PII_XF_MASK || H.xf_kind[t] == PII_XF_KEEP;
        tok_len[t] = same_len ? XF_SAME_LEN : tok_off[t + 1] - tok_off[t];
    }
    tok += "\n";               // the re-scan window separator (k_win_redact piece source)
    R.nl_off = (uint32_t)tok.size() - 1;
    tok.append(32, '\0');     // k_redact reads aligned 16-byte windows past a token's end
    // SCAN groups >= 1
    struct GroupTabs {
        std::vector<uint16_t> td, dacc, npair;
        std::vector<uint32_t> cmap4;
    };
    std::vector<GroupTabs> gt;
    {
        const int64_t n_extra = meta[14];
        if (n_extra < 0 || n_extra + 1 > SCAN_GROUPS_MAX) return "too many SCAN groups";
        const Section* gs = find("scan.groups");
        if (n_extra > 0 && (!gs || gs->bytes < (size_t)n_extra * 32)) return "SCAN group table missing";
        for (int64_t q = 1; q <= n_extra; ++q) {
            const int64_t* gm = reinterpret_cast<const int64_t*>(gs->data) + 4 * (q - 1);
            const std::string nm = "scan.g" + std::to_string(q);
            const Section *sc = find(nm + ".cmap"), *st = find(nm + ".trans"), *sa = find(nm + ".accid");
            HostGroup h{};
            GroupTabs g;
            h.SD = (int)gm[0];
            h.CD = (int)gm[1];
            h.CDs = (h.CD + 1) & ~1;
            if (!sc || !st || !sa || st->bytes != (size_t)h.SD * h.CD * 2 || sa->bytes != st->bytes || sc->bytes != 256)
                return "SCAN group tables malformed";
            // a table past 64 KiB of LDS addresses is WIDE: rows padded to a multiple of 4 entries (8-byte
            // aligned), entries hold the row offset / 2, so 16-bit entries reach 128 KiB (and the u16
            // transition index of an event, 64k entries)
            if (SCAN_TD_BASE + (size_t)h.SD * h.CDs * 2 + 4 + SCAN_SPREAD_BYTES > 65536) {
                h.CDs = (h.CD + 3) & ~3;
                h.dsh = 1;
                if ((size_t)h.SD * h.CDs > 65536) return "a SCAN group exceeds 128 KiB of LDS";
            }
            const uint32_t tkb = SCAN_TD_BASE + (uint32_t)(h.SD * h.CDs) * 2;
            h.lds = tkb + 4 + SCAN_SPREAD_BYTES;                // + the K stub's row (2 entries), spread masks
            if (h.lds + FIX_LDS > 160 * 1024) return "a SCAN group exceeds the LDS";
            g.td.assign((size_t)h.SD * h.CDs, 0);
            g.dacc.assign((size_t)h.SD * h.CDs, 0);
            if (gm[2] < 0 || gm[2] >= h.SD) return "SCAN group start state out of range";
            relayout(reinterpret_cast<const uint16_t*>(st->data), reinterpret_cast<const uint16_t*>(sa->data), h.SD,
                     h.CD, h.CDs, (int)gm[2], g.td.data(), g.dacc.data(), h.dsh);
            g.cmap4.resize(256);
            // class words of a group >= 1: the D half only (its K is the stub, stepped at tk_base)
            for (int b = 0; b < 256; ++b) g.cmap4[b] = SCAN_TD_BASE + 2u * sc->data[b];
            H.groups.push_back(h);
            gt.push_back(std::move(g));
        }
    }
    std::vector<uint16_t> d_npair(dacc.size()), k_grp(kacc.size());
    std::vector<uint32_t> d_na(dacc.size());
    {
        const uint32_t* off = u32("scan.d.acc_off");
        for (size_t i = 0; i < dacc.size(); ++i) d_npair[i] = (uint16_t)(off[dacc[i] + 1] - off[dacc[i]]);
        for (size_t i = 0; i < kacc.size(); ++i) k_grp[i] = kacc[i] ? k_acc_min[kacc[i]] : (uint16_t)KW_NONE;
        for (auto& g : gt) {
            g.npair.resize(g.dacc.size());
            for (size_t i = 0; i < g.dacc.size(); ++i) g.npair[i] = (uint16_t)(off[g.dacc[i] + 1] - off[g.dacc[i]]);
        }
        for (size_t i = 0; i < dacc.size(); ++i) d_na[i] = d_npair[i] | (uint32_t)dacc[i] << 16;
    }
    // one buffer holding every table, 256-byte aligned sections (16 spare bytes after each)
    auto put = [&](const void* src, size_t bytes) {
        const size_t o = (H.packed.size() + 255) & ~(size_t)255;
        H.packed.resize(o + bytes + 16, 0);
        if (bytes) std::memcpy(H.packed.data() + o, src, bytes);
        return o;
    };
    auto putv = [&](const auto& v) { return put(v.data(), v.size() * sizeof(v[0])); };
    auto putsec = [&](const char* nm) { return put(find(nm)->data, find(nm)->bytes); };
    H.off[TB_CMAP4] = putv(cmap4);
    H.off[TB_TD] = putv(td);
    H.off[TB_TK] = putv(tk);
    H.off[TB_D_ACCID] = putv(dacc);
    H.off[TB_D_ACC_OFF] = putsec("scan.d.acc_off");
    H.off[TB_D_ACC_IDS] = putsec("scan.d.acc_ids");
    H.off[TB_K_ACCID] = putv(kacc);
    H.off[TB_K_ACC_MIN] = putv(k_acc_min);
    H.off[TB_D_NPAIR] = putv(d_npair);
    H.off[TB_K_GRP] = putv(k_grp);
    H.off[TB_D_NA] = putv(d_na);
    static const char* const plain[] = {"det.type", "det.validator", "det.lik", "det.exidx", "det.first_desc",
                                        "hot.rule", "hot.dfa_desc", "var.enabled", "var.minlik", "var.rule_off",
                                        "var.rule_ids", "var.excl_off", "var.excl_ids"};
    static_assert(sizeof(plain) / sizeof(plain[0]) == TB_EXCL_IDS - TB_DET_TYPE + 1, "the blob sections placed as they are");
    for (int i = 0; i <= TB_EXCL_IDS - TB_DET_TYPE; ++i) H.off[TB_DET_TYPE + i] = putsec(plain[i]);
    H.off[TB_TOK_OFF] = putv(tok_off);
    H.off[TB_TOK_BYTES] = putv(tok);
    H.off[TB_TOK_LEN] = putv(tok_len);
    H.off[TB_XF_KIND] = putv(H.xf_kind);
    H.off[TB_XF_MASK] = putv(xf_maskp);
    static const uint16_t stub[2] = {0, 0};          // a group's K: one row, never accepting
    for (size_t q = 0; q < gt.size(); ++q) {
        size_t* o = H.groups[q].off;
        o[GT_CMAP4] = putv(gt[q].cmap4);
        o[GT_TD] = putv(gt[q].td);
        o[GT_TK] = put(stub, 4);
        o[GT_D_ACCID] = putv(gt[q].dacc);
        o[GT_K_ACCID] = put(stub, 4);
        o[GT_D_NPAIR] = putv(gt[q].npair);
    }
    if (H.xf_hash) {
        H.off[TB_HASH_KEY] = put(xs_hkey->data, xs_hkey->bytes);
        H.off[TB_HASH_MID] = put(xs_hmid->data, xs_hmid->bytes);
    }
    if (H.excl_general) {
        H.off[TB_XG_OFF] = put(xs_goff->data, xs_goff->bytes);
        H.off[TB_XG_IDS] = put(xs_gids->data, xs_gids->bytes);
        H.off[TB_XG_IDX] = put(xs_gidx->data, xs_gidx->bytes);
    }
    if (R.n_dacc >= 65535) return "too many SCAN accept sets";
    // per-kernel LDS images
    auto sec = [&](const char* nm) { return std::make_pair((const void*)find(nm)->data, (size_t)find(nm)->bytes); };
    const uint16_t* ptrans = u16("pool.trans");
    const uint8_t* pflags = find("pool.flags")->data;
    const uint8_t* pcmap = find("pool.cmap")->data;
    DfaPool fp, hp;
    const int32_t* fdesc = i32("det.first_desc");
    // absorbed match starts: the patterns' PRE states (absent in older blobs: nothing is dropped)
    const Section* s_pre = find("det.first_pre");
    if (s_pre && s_pre->bytes < (size_t)R.P * 4) return "det.first_pre is too short";
    if (!knobs.first_drop) s_pre = nullptr;
    auto fpre = [&](int p) { return s_pre ? reinterpret_cast<const int32_t*>(s_pre->data)[p] : -1; };
    for (int p = 0; p < R.P; ++p)
        if (fpre(p) >= fdesc[8 * p + 7]) return "det.first_pre names a state past its automaton";
    bool fits = true;
    for (int p = 0; p < R.P; ++p) fits &= add_dfa(fp, fdesc + 8 * p, ptrans, pflags, pcmap, fpre(p));
    const int32_t* hdesc = i32("hot.dfa_desc");
    for (int h = 0; h < R.n_hot; ++h) fits &= add_dfa(hp, hdesc + 8 * h, ptrans, pflags, pcmap);
    if (!fits) return "a FIRST/HOT automaton has more than 16384 states";
    if (hp.desc.empty()) hp.desc.assign(8, 0);
    const size_t n_keys = (size_t)R.V * R.T;
    const ListTab rl = dedup_lists(u32("var.rule_off"), u16("var.rule_ids"), n_keys);
    const ListTab xl = dedup_lists(u32("var.excl_off"), u16("var.excl_ids"), n_keys);
    const uint32_t aux = rl.w | xl.w << 3;
    H.lists_cl = rl.w != 0 || xl.w != 0;
    // per type: every hotword rule it has in any context variant (k_win_eval's resident bits)
    std::vector<uint32_t> thot(std::max(R.T, 1), 0u);
    {
        const uint32_t* ro = u32("var.rule_off");
        const uint16_t* ri = u16("var.rule_ids");
        for (int v = 0; v < R.V; ++v)
            for (int t = 0; t < R.T; ++t)
                for (uint32_t q = ro[v * R.T + t]; q < ro[v * R.T + t + 1]; ++q)
                    if (ri[q] < 32) thot[t] |= 1u << ri[q];     // k_win_* cache the first WHOT_BITS
    }
    ImageParts pf(FI_N), pe(EV_N), ps(SE_N), pw(WS_N);
    pf[FI_TRANS] = part(fp.trans);
    pf[FI_CMAP] = part(fp.cmap);
    pf[FI_DESC] = part(fp.desc);
    pe[EV_TRANS] = pw[WS_TRANS] = part(hp.trans);
    pe[EV_CMAP] = pw[WS_CMAP] = part(hp.cmap);
    pe[EV_HDESC] = pw[WS_HDESC] = part(hp.desc);
    pe[EV_HRULE] = pw[WS_HRULE] = sec("hot.rule");
    pe[EV_DTYPE] = pw[WS_DTYPE] = ps[SE_DTYPE] = sec("det.type");
    pe[EV_DVAL] = sec("det.validator");
    pe[EV_DLIK] = pw[WS_DLIK] = sec("det.lik");
    pe[EV_ROFF] = pw[WS_ROFF] = part(rl.ix);
    pe[EV_RLOFF] = pw[WS_RLOFF] = part(rl.loff);
    pe[EV_RIDS] = pw[WS_RIDS] = part(rl.ids);
    pe[EV_THOT] = part(thot);
    pw[WS_VEN] = ps[SE_VEN] = sec("var.enabled");
    pw[WS_VMIN] = ps[SE_VMIN] = sec("var.minlik");
    pw[WS_DEX] = ps[SE_DEX] = sec("det.exidx");
    pw[WS_XOFF] = ps[SE_XOFF] = part(xl.ix);
    pw[WS_XLOFF] = ps[SE_XLOFF] = part(xl.loff);
    pw[WS_XIDS] = ps[SE_XIDS] = part(xl.ids);
    pw[WS_TOKOFF] = ps[SE_TOKOFF] = part(tok_len);
    static const char* img_bad = "rule table upload failed";
    if (!pack_image(pw, aux, H.img_wsel) || !pack_image(pf, 0, H.img_first) || !pack_image(pe, aux, H.img_eval) ||
        !pack_image(ps, aux, H.img_sel))
        return img_bad;
    if (H.excl_text) {
        ImageParts px(TX_N);
        px[TX_TRANS] = part(xp.trans);
        px[TX_CMAP] = part(xp.cmap);
        px[TX_DESC] = part(xp.desc);
        px[TX_RULE] = sec("xt.rule");
        px[TX_DTYPE] = sec("det.type");
        px[TX_OFF] = part(xtl.ix);
        px[TX_IDS] = part(xtl.ids);
        px[TX_LOFF] = part(xtl.loff);
        if (!pack_image(px, xtl.w, H.img_xtext)) return img_bad;
    }
    if (H.img_first.global) {
        DfaPool hf;
        const uint32_t ph = pack_first_hot(knobs, R.P, fdesc, ptrans, pflags, pcmap, fpre, hf);
        if (ph > 0) {
            ImageParts parts(FI_N);
            parts[FI_TRANS] = part(hf.trans);
            parts[FI_CMAP] = part(hf.cmap);
            parts[FI_DESC] = part(hf.desc);
            if (!pack_image(parts, 0, H.img_first_hot)) return img_bad;
            H.first_p_hot = ph;
        }
    }
    // the list-less variants of a pair-kernel image past IMG_LDS_SPLIT (the kernel reads the lists from
    // L2): kept only when they fit where the full image did not
    if (H.img_eval.li.total > IMG_LDS_SPLIT) {
        pe[EV_ROFF] = pe[EV_RLOFF] = pe[EV_RIDS] = {nullptr, 0};
        if (!pack_image(pe, 0, H.img_eval_rg)) return img_bad;
        if (H.img_eval_rg.global) H.img_eval_rg = HostImage{};
    }
    if (H.img_sel.li.total > IMG_LDS_SPLIT) {
        ps[SE_XOFF] = ps[SE_XLOFF] = ps[SE_XIDS] = {nullptr, 0};
        if (!pack_image(ps, 0, H.img_sel_rg)) return img_bad;
        if (H.img_sel_rg.global || H.img_sel_rg.li.total > 64 * 1024) H.img_sel_rg = HostImage{};   // (no gain: keep the full image)
    }
    H.scan_lds = SCAN_TD_BASE + (size_t)(R.SD * R.CDs / 2) * 4 + (size_t)(R.SK * R.CKs / 2) * 4 + SCAN_SPREAD_BYTES;
    if (H.scan_lds > 160 * 1024) return "SCAN tables do not fit in LDS";
    return nullptr;
}

}  // namespace
