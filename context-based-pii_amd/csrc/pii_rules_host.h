// pii_rules_host.h - everything pii_engine_create does before its first HIP call: blob parsing, the
// derived host tables, the packed rules buffer, the kernels' LDS images.  Plain C++17 (no HIP header),
// so a host compiler alone builds and runs it (tests/rules_host_main.cpp, under the sanitizers).
//
// build_host_rules(blob, knobs) -> a HostRules value, or the message of the first defect it met.
// Section bytes are read through View<T> alone (Blob::view: presence, element type, whole elements,
// count); what a table's entries point at is checked by check_lists / check_dfa / check_scan before
// anything follows them.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pii_engine.h"
#include "pii_fpe.h"
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

// ------------------------------------------------------------------------------- section views
// a defect: its message goes to HostRules::defect, the stage that met it returns false
struct Why {
    std::string& msg;
    bool operator()(std::string m) const {
        msg = std::move(m);
        return false;
    }
};

// a section's elements: the one form in which section bytes are read
template <class T>
struct View {
    const T* p = nullptr;
    size_t n = 0;
    const T* data() const { return p; }
    size_t size() const { return n; }
    const T& operator[](size_t i) const { return p[i]; }
    View sub(size_t at, size_t len) const { return {p + at, len}; }   // (of a range the caller has checked)
};

// the blob's dtype codes (compiler.py _DT)
template <class T> struct DType;
template <> struct DType<uint8_t> { static constexpr uint32_t code = 1; static constexpr const char* name = "u8"; };
template <> struct DType<uint16_t> { static constexpr uint32_t code = 2; static constexpr const char* name = "u16"; };
template <> struct DType<uint32_t> { static constexpr uint32_t code = 3; static constexpr const char* name = "u32"; };
template <> struct DType<int32_t> { static constexpr uint32_t code = 4; static constexpr const char* name = "i32"; };
template <> struct DType<int64_t> { static constexpr uint32_t code = 5; static constexpr const char* name = "i64"; };

struct Blob {
    std::vector<Section> secs;
    Why bad;
    const Section* find(const std::string& nm) const {
        for (auto& s : secs)
            if (s.name == nm) return &s;
        return nullptr;
    }
    bool has(const std::string& nm) const { return find(nm) != nullptr; }
    // the section as elements of T: it is there, holds T (its dtype code) and whole elements
    template <class T>
    bool view(const std::string& nm, View<T>& v) const {
        const Section* s = find(nm);
        if (!s) return bad("a required section is missing: " + nm);
        if (s->dtype != DType<T>::code) return bad(nm + " does not hold " + DType<T>::name + " values");
        if (s->bytes % sizeof(T) != 0) return bad(nm + " does not hold whole " + DType<T>::name + " values");
        v.p = reinterpret_cast<const T*>(s->data);
        v.n = (size_t)(s->bytes / sizeof(T));
        return true;
    }
    // ... and exactly `count` of them: "<section> does not hold <what>"
    template <class T>
    bool view(const std::string& nm, View<T>& v, size_t count, const char* what) const {
        return view(nm, v) && (v.n == count || bad(nm + " does not hold " + what));
    }
};

// ------------------------------------------------------------------------------- the three checkers
// A list table: off[keys + 1] into ids, every id (& mask) below `bound`.
struct ListNames {
    const char *off, *ids, *count, *id, *table;   // "<ids> names <id> past <table>"
};
inline bool check_lists(View<uint32_t> off, View<uint16_t> ids, size_t keys, uint16_t mask, size_t bound,
                        const ListNames& nm, const Why& bad) {
    if (off.n != keys + 1) return bad(std::string(nm.off) + " does not hold " + nm.count);
    if (off[0] != 0) return bad(std::string(nm.off) + " does not start at 0");
    for (size_t k = 0; k < keys; ++k)
        if (off[k] > off[k + 1]) return bad(std::string(nm.off) + " is not ascending");
    if (off[keys] > ids.n) return bad(std::string(nm.ids) + " is shorter than its offsets");
    for (uint32_t q = 0; q < off[keys]; ++q)
        if ((size_t)(ids[q] & mask) >= bound) return bad(std::string(nm.ids) + " names " + nm.id + " past " + nm.table);
    return true;
}

// A pool automaton: its descriptor `d` (8 words: trans / flags / cmap offsets, columns = classes + end of
// text, three start states, states) into the pools.
struct BlobPool {
    View<uint16_t> trans;
    View<uint8_t> flags, cmap;
};
struct PoolNames {
    const char *desc, *trans, *flags, *cmap;
    const char* many;   // the message for more than DFA_STATE_MASK + 1 states
};
inline bool check_dfa(View<int32_t> d, const BlobPool& pl, const PoolNames& nm, const Why& bad) {
    const int64_t nc = d[3], ns = d[7];
    const std::string ds = nm.desc;
    if (nc < 2 || nc > 256 || ns < 1) return bad(ds + " holds an automaton of impossible size");
    if (ns > (int64_t)pii::DFA_STATE_MASK + 1) return bad(nm.many);
    if (d[0] < 0 || (uint64_t)d[0] + (uint64_t)(ns * nc) > pl.trans.n) return bad(ds + " points past " + nm.trans);
    if (d[1] < 0 || (uint64_t)d[1] + (uint64_t)ns > pl.flags.n) return bad(ds + " points past " + nm.flags);
    if (d[2] < 0 || (uint64_t)d[2] + 256 > pl.cmap.n) return bad(ds + " points past " + nm.cmap);
    for (int i = 4; i <= 6; ++i)
        if (d[i] < 0 || d[i] >= ns) return bad(ds + " holds a start state past its automaton");
    for (int64_t i = 0; i < ns * nc; ++i)
        if (pl.trans[d[0] + i] >= ns) return bad(std::string(nm.trans) + " holds a state past its automaton");
    for (int c = 0; c < 256; ++c)
        if (pl.cmap[d[2] + c] >= nc - 1) return bad(std::string(nm.cmap) + " holds a class past its automaton");
    return true;
}

// A SCAN table: S states x C columns (classes + end of text) of destination | accept << 15, an accept set
// id per entry (0 = none; `n_sets` sets, the empty one included), a start state, a class per byte.
struct ScanNames {
    std::string trans, accid, cmap;
    const char* start;   // the whole message
};
template <class ClassOf>
bool check_scan(View<uint16_t> trans, View<uint16_t> accid, int64_t S, int64_t C, int64_t start, size_t n_sets, ClassOf cls,
                const ScanNames& nm, const Why& bad) {
    static const char* per = " does not hold one entry per state and class";
    if (trans.n != (uint64_t)(S * C)) return bad(nm.trans + per);
    if (accid.n != trans.n) return bad(nm.accid + per);
    if (start < 0 || start >= S) return bad(nm.start);
    for (size_t i = 0; i < trans.n; ++i) {
        if ((trans[i] & 0x7fff) >= S) return bad(nm.trans + " holds a state past its automaton");
        if (accid[i] >= n_sets) return bad(nm.accid + " names an accept set past the accept sets");
    }
    for (int b = 0; b < 256; ++b)
        if ((int64_t)cls(b) >= C - 1) return bad(nm.cmap + " holds a class past its automaton");
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
// d: a descriptor check_dfa passed; pre: a FIRST automaton's PRE state (absorbed match starts,
// first_begin), -1 = none
inline void add_dfa(DfaPool& dp, View<int32_t> d, const BlobPool& pl, int32_t pre = -1) {
    const int32_t nc = d[3], ns = d[7];
    int32_t nd[8];
    std::memcpy(nd, d.p, sizeof(nd));
    // LDS bank stagger (32 banks x 4 B): a pair kernel's wavefront runs many patterns' automata over
    // the same text bytes, so automaton k's transition table starts at bank k mod 32 and its class map
    // 4 bytes after the previous map's end (byte c of every map would otherwise sit in one bank)
    const size_t k = dp.desc.size() / 8;
    while (dp.trans.size() % 64 != (2 * k) % 64) dp.trans.push_back(0);
    nd[0] = (int32_t)dp.trans.size();
    nd[1] = pre < 0 ? 0 : pre + 1;
    nd[2] = (int32_t)dp.cmap.size();
    for (size_t i = 0; i < (size_t)ns * nc; ++i) {
        const uint16_t dst = pl.trans[d[0] + i];
        dp.trans.push_back((uint16_t)(dst | ((pl.flags[d[1] + dst] & 3u) << 14)));
    }
    dp.cmap.insert(dp.cmap.end(), pl.cmap.p + d[2], pl.cmap.p + d[2] + 256);
    dp.cmap.insert(dp.cmap.end(), 4, (uint8_t)0);
    dp.desc.insert(dp.desc.end(), nd, nd + 8);
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
// off / ids: a table check_lists passed, of off.n - 1 keys
inline ListTab dedup_lists(View<uint32_t> off, View<uint16_t> ids) {
    const size_t n_keys = off.n - 1;
    ListTab t;
    if (n_keys <= LIST_DEDUP_KEYS) {
        t.w = 0;
        t.ix.push_back(0);
        t.loff.assign(off.p, off.p + n_keys + 1);
        t.ids.assign(ids.p, ids.p + off[n_keys]);
        if (t.ids.empty()) t.ids.push_back(0);
        return t;
    }
    std::map<std::vector<uint16_t>, uint32_t> uniq;
    std::vector<uint32_t> num(n_keys);
    t.loff.push_back(0);
    for (size_t i = 0; i < n_keys; ++i) {
        std::vector<uint16_t> l(ids.p + off[i], ids.p + off[i + 1]);
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
// hash type keep their layout), the general exclusion tables after those (likewise), the FPE tables after
// those (likewise); the text exclusion rules live in their kernel's image alone
enum { TB_CMAP4, TB_TD, TB_TK, TB_D_ACCID, TB_D_ACC_OFF, TB_D_ACC_IDS, TB_K_ACCID, TB_K_ACC_MIN, TB_D_NPAIR, TB_K_GRP,
       TB_D_NA, TB_DET_TYPE, TB_DET_VAL, TB_DET_LIK, TB_DET_EXIDX, TB_FIRST_DESC, TB_HOT_RULE, TB_HOT_DESC,
       TB_VAR_ENABLED, TB_VAR_MINLIK, TB_RULE_OFF, TB_RULE_IDS, TB_EXCL_OFF, TB_EXCL_IDS, TB_TOK_OFF, TB_TOK_BYTES,
       TB_TOK_LEN, TB_XF_KIND, TB_XF_MASK, TB_HASH_KEY, TB_HASH_MID, TB_XG_OFF, TB_XG_IDS, TB_XG_IDX, TB_FPE, TB_FPE_KEY,
       TB_FPE_ALPHA, TB_FPE_TE0, TB_N };
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
    bool xf_src = false, xf_mask = false, xf_hash = false, xf_fpe = false;
    uint32_t fpe_nkeys = 0;            // the key records of xf.fpe_key (<= XF_FPE_KEYS_MAX)
    bool window_ok = false;
    bool window_xg_ok = false;         // general / text exclusion rules alone took window_ok (meta[15]; absent: no)
    // general exclusion rules (var.xg_off / var.xg_ids / det.xgidx): k_exclude decides them, the
    // streaming lists are empty; excl_nx = its excluder patterns
    bool excl_general = false;
    int excl_nx = 0;
    bool excl_lists = false;           // some (variant, type) has an exclude_info_types list: k_exclude's phases run
    // text exclusion rules (var.xt_off / var.xt_ids / xt.*): k_excl_text decides them (img_xtext)
    bool excl_text = false;
    std::string defect;                // the message build_host_rules returned, where it composed one
};

// entry (row, class) = address of the destination row | accept | accept of the destination's
// end-of-text transition (class C-1) << 1, so k_scan resets at an utterance start without
// reading the end-of-text entry
// (k_scan: rows are placed with the START state first -- row = pos(state) -- and entries are the
// destination row's byte offset from the table base, so a reset is "row 0"; the class words carry
// the table bases; accept-id tables follow the same placement)
// s / acc: a table check_scan passed
inline void relayout(View<uint16_t> s, View<uint16_t> acc, int S, int C, int Cs, int start, uint16_t* t, uint16_t* a,
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
uint32_t pack_first_hot(const RuleKnobs& k, int P, View<int32_t> fdesc, const BlobPool& pl, Pre fpre, DfaPool& hf) {
    const size_t big = k.first_hot_big, budget = k.first_hot_lds;
    const uint32_t cap_p = std::min<uint32_t>((uint32_t)P, k.first_hot);
    auto bytes_with = [&](size_t tr, size_t cm, size_t np) {
        return ((tr * 2 + 15) & ~(size_t)15) + ((cm + 260 + 15) & ~(size_t)15) + ((np * 32 + 15) & ~(size_t)15);
    };
    uint32_t ph = 0;
    size_t trans_n = 0, cmap_n = 0;
    for (uint32_t p = 0; p < cap_p; ++p) {
        const View<int32_t> d = fdesc.sub(8 * p, 8);
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
        const View<int32_t> d = fdesc.sub(8 * p, 8);
        const size_t dfa = (size_t)d[7] * d[3] * 2, tr = hf.trans.size() + 64 + (size_t)d[7] * d[3];
        if ((big && dfa > big) || bytes_with(tr, hf.cmap.size(), ph) > budget) {
            hf.desc.insert(hf.desc.end(), 8, 0);          // columns 0: not resident
            continue;
        }
        add_dfa(hf, d, pl, fpre((int)p));
    }
    return ph;
}

// ------------------------------------------------------------------------------- the stages
// What the stages hand on beside HostRules: the checked section views and the tables derived from them.
struct CoreSecs {
    View<int64_t> meta;
    View<uint16_t> cmap2, d_trans, d_accid, d_acc_ids, k_trans, k_accid, k_acc_ids, det_type, rule_ids, excl_ids, kw_type;
    View<uint32_t> d_acc_off, k_acc_off, rule_off, excl_off;
    View<uint8_t> det_val, det_lik, det_exidx, var_enabled, var_minlik, kw_always, type_names;
    View<int32_t> first_desc, hot_rule, hot_desc;
    BlobPool pool;
    int d_start = 0, k_start = 0;   // as the blob numbers the states (R's are row offsets: 0)
    size_t keys = 0;                // V * T
};
struct HostExcl {
    View<uint32_t> xg_off;          // general: placed in the rules buffer as they are
    View<uint16_t> xg_ids;
    View<uint8_t> xg_idx;
    View<int32_t> xt_rule;          // text: the image's parts
    DfaPool xp;
    ListTab xtl;
};
struct HostXf {
    std::vector<uint32_t> maskp, tok_off, tok_len;
    std::string tok;
    View<uint32_t> hash_key, hash_mid;
    View<uint32_t> fpe, fpe_key, fpe_alpha;
    std::vector<uint32_t> fpe_te0;  // the AES table (fpe_te0), built here
};
struct GroupTabs {
    std::vector<uint16_t> td, dacc, npair;
    std::vector<uint32_t> cmap4;
};
struct HostScan {
    std::vector<uint16_t> td, tk, dacc, kacc, k_acc_min, d_npair, k_grp;
    std::vector<uint32_t> cmap4, d_na;
    std::vector<GroupTabs> gt;
};

// The required sections, each with its count, and everything a later stage or a kernel follows out of
// them: dimensions, list tables, the D and K SCAN tables, the FIRST and HOT automata, types.
inline bool read_core(const Blob& B, CoreSecs& c, HostRules& H) {
    const Why& bad = B.bad;
    RulesDev& R = H.R;
    if (!B.view("meta", c.meta)) return false;
    if (c.meta.n < 15) return bad("meta does not hold 15 values");
    int* const dims[] = {&R.P, &R.G, &R.T, &R.V, &R.SD, &R.CD, &R.d_start, &R.SK, &R.CK, &R.k_start, &R.n_hot, &R.min_len};
    for (int i = 0; i < 12; ++i) {
        if (i != 11 && (c.meta[i] < 0 || c.meta[i] > (1 << 30))) return bad("meta holds a dimension out of range");
        *dims[i] = (int)c.meta[i];
    }
    R.min_len = (int)std::clamp<int64_t>(c.meta[11], 1, 1 << 30);
    H.window_ok = c.meta[13] != 0;
    H.window_xg_ok = !H.window_ok && c.meta.n > 15 && c.meta[15] != 0;
    if (R.P > 65535) return bad("too many detector patterns");
    // scan table entries are 16-bit LDS byte addresses (k_scan layout: class map, D rows, K rows);
    // rows are padded to an even class count so every row address is a multiple of 4 and bit 1 of
    // an entry is free for the destination's end-of-text accept
    R.CDs = (R.CD + 1) & ~1;
    R.CKs = (R.CK + 1) & ~1;
    R.dsh = 0;
    if (SCAN_TD_BASE + ((uint64_t)R.SD * R.CDs + (uint64_t)R.SK * R.CKs) * 2 > 65536) return bad("SCAN tables exceed 64 KiB of LDS");
    if (R.T > 65535) return bad("too many types");
    const size_t P = R.P, T = R.T, V = R.V, G = R.G, n_hot = R.n_hot, keys = c.keys = V * T;
    if (!B.view("types.names", c.type_names)) return false;
    {
        const char* p = reinterpret_cast<const char*>(c.type_names.p);
        for (size_t i = 0; i < c.type_names.n;) {
            const size_t l = strnlen(p + i, c.type_names.n - i);
            H.names.emplace_back(p + i, l);
            i += l + 1;
        }
        if (H.names.size() != T) return bad("type table mismatch");
    }
    // (a table without entries is written with one filler entry: kw.*, hot.*)
    const bool there =
        B.view("scan.cmap2", c.cmap2, 256, "one class pair per byte") && B.view("scan.d.trans", c.d_trans) &&
        B.view("scan.d.accid", c.d_accid) && B.view("scan.d.acc_off", c.d_acc_off) && B.view("scan.d.acc_ids", c.d_acc_ids) &&
        B.view("scan.k.trans", c.k_trans) && B.view("scan.k.accid", c.k_accid) && B.view("scan.k.acc_off", c.k_acc_off) &&
        B.view("scan.k.acc_ids", c.k_acc_ids) && B.view("det.type", c.det_type, P, "one type per pattern") &&
        B.view("det.validator", c.det_val, P, "one validator per pattern") &&
        B.view("det.lik", c.det_lik, P, "one likelihood per pattern") &&
        B.view("det.exidx", c.det_exidx, P, "one excluder slot per pattern") &&
        B.view("det.first_desc", c.first_desc, P * 8, "one descriptor per pattern") &&
        B.view("hot.rule", c.hot_rule, std::max<size_t>(1, n_hot) * 4, "one entry per hotword rule") &&
        B.view("hot.dfa_desc", c.hot_desc, std::max<size_t>(1, n_hot) * 8, "one descriptor per hotword rule") &&
        B.view("pool.trans", c.pool.trans) && B.view("pool.flags", c.pool.flags) && B.view("pool.cmap", c.pool.cmap) &&
        B.view("var.enabled", c.var_enabled, keys, "one flag per variant and type") &&
        B.view("var.minlik", c.var_minlik, V, "one likelihood per variant") && B.view("var.rule_off", c.rule_off) &&
        B.view("var.rule_ids", c.rule_ids) && B.view("var.excl_off", c.excl_off) && B.view("var.excl_ids", c.excl_ids) &&
        B.view("kw.type", c.kw_type, std::max<size_t>(1, G), "one type per context group") &&
        B.view("kw.always", c.kw_always, std::max<size_t>(1, G), "one flag per context group");
    if (!there) return false;
    for (size_t p = 0; p < P; ++p)
        if (c.det_type[p] >= T) return bad("det.type names a type past the type table");
    for (size_t g = 0; g < G; ++g) {
        if (c.kw_type[g] >= T) return bad("kw.type names a type past the type table");
        H.kw_type.push_back(c.kw_type[g]);
    }
    // accept sets: the key count is the table's own
    R.n_dacc = c.d_acc_off.n ? (uint32_t)(c.d_acc_off.n - 1) : 0;
    R.n_kacc = c.k_acc_off.n ? (uint32_t)(c.k_acc_off.n - 1) : 0;
    if (R.n_dacc >= 65535) return bad("too many SCAN accept sets");
    static const char* vt = "V*T+1 offsets";
    if (!check_lists(c.d_acc_off, c.d_acc_ids, R.n_dacc, 0xffff, P,
                     {"scan.d.acc_off", "scan.d.acc_ids", "an offset", "a pattern", "the pattern table"}, bad) ||
        !check_lists(c.k_acc_off, c.k_acc_ids, R.n_kacc, 0xffff, G,
                     {"scan.k.acc_off", "scan.k.acc_ids", "an offset", "a context group", "the context groups"}, bad) ||
        !check_lists(c.rule_off, c.rule_ids, keys, 0xffff, n_hot,
                     {"var.rule_off", "var.rule_ids", vt, "a hotword rule", "the rule table"}, bad) ||
        !check_lists(c.excl_off, c.excl_ids, keys, 0xffff, T,
                     {"var.excl_off", "var.excl_ids", vt, "a type", "the type table"}, bad))
        return false;
    c.d_start = R.d_start;
    c.k_start = R.k_start;
    if (!check_scan(c.d_trans, c.d_accid, R.SD, R.CD, c.d_start, R.n_dacc, [&](int b) { return c.cmap2[b] & 0xff; },
                    {"scan.d.trans", "scan.d.accid", "scan.cmap2", "meta names a D start state past its automaton"}, bad) ||
        !check_scan(c.k_trans, c.k_accid, R.SK, R.CK, c.k_start, R.n_kacc, [&](int b) { return c.cmap2[b] >> 8; },
                    {"scan.k.trans", "scan.k.accid", "scan.cmap2", "meta names a K start state past its automaton"}, bad))
        return false;
    R.d_start = R.k_start = 0;                                     // row offsets: the start rows are first
    static const char* many = "a FIRST/HOT automaton has more than 16384 states";
    for (size_t p = 0; p < P; ++p)
        if (!check_dfa(c.first_desc.sub(8 * p, 8), c.pool, {"det.first_desc", "pool.trans", "pool.flags", "pool.cmap", many}, bad))
            return false;
    for (size_t h = 0; h < n_hot; ++h)   // (without hotword rules the one all-zero row is no automaton)
        if (!check_dfa(c.hot_desc.sub(8 * h, 8), c.pool, {"hot.dfa_desc", "pool.trans", "pool.flags", "pool.cmap", many}, bad))
            return false;
    R.kw_always_min = KW_NONE;
    for (size_t g = 0; g < G; ++g)
        if (c.kw_always[g]) {
            R.kw_always_min = (int)g;
            break;
        }
    int ne = 0;
    for (size_t p = 0; p < P; ++p)
        if (c.det_exidx[p] != 0xff) ne = std::max(ne, c.det_exidx[p] + 1);
    if (ne > NE_MAX) return bad("too many excluder patterns");
    R.NE = ne;
    return true;
}

// general exclusion rules: the three sections together or not at all, beside empty streaming lists
inline bool read_general_exclusion(const Blob& B, const CoreSecs& c, HostExcl& x, HostRules& H) {
    const Why& bad = B.bad;
    const int present = B.has("var.xg_off") + B.has("var.xg_ids") + B.has("det.xgidx");
    if (!present) return true;
    if (present != 3) return bad("general exclusion sections are not all present");
    if (!B.view("var.xg_off", x.xg_off) || !B.view("var.xg_ids", x.xg_ids) ||
        !B.view("det.xgidx", x.xg_idx, (size_t)H.R.P, "one index per pattern") ||
        !check_lists(x.xg_off, x.xg_ids, c.keys, XG_PARTIAL - 1, (size_t)H.R.T,
                     {"var.xg_off", "var.xg_ids", "V*T+1 offsets", "a type", "the type table"}, bad))
        return false;
    int nx = 0;
    for (size_t p = 0; p < x.xg_idx.n; ++p)
        if (x.xg_idx[p] != 0xff) {
            if (x.xg_idx[p] >= NX_MAX) return bad("det.xgidx holds an index past the limit");
            nx = std::max(nx, x.xg_idx[p] + 1);
        }
    if (H.R.NE != 0 || c.excl_off[c.keys] != 0) return bad("general exclusion sections beside streaming exclusion lists");
    H.excl_general = true;
    H.excl_nx = nx;
    H.excl_lists = x.xg_off[c.keys] != 0;
    return true;
}

// text exclusion rules: the seven sections together or not at all, and only beside the general ones
inline bool read_text_exclusion(const Blob& B, const CoreSecs& c, HostExcl& x, HostRules& H) {
    const Why& bad = B.bad;
    int present = 0;
    for (const char* nm : {"var.xt_off", "var.xt_ids", "xt.rule", "xt.desc", "xt.trans", "xt.flags", "xt.cmap"})
        present += B.has(nm);
    if (!present) return true;
    if (present != 7) return bad("text exclusion sections are not all present");
    if (!H.excl_general) return bad("text exclusion sections without the general exclusion sections");
    View<uint32_t> off;
    View<uint16_t> ids;
    View<int32_t> desc;
    BlobPool pl;
    if (!B.view("xt.rule", x.xt_rule)) return false;
    const size_t nr = x.xt_rule.n / 4;
    if (nr == 0 || x.xt_rule.n % 4 != 0 || nr > 65535) return bad("xt.rule does not hold whole rules");
    if (!B.view("xt.desc", desc, nr * 8, "one descriptor per rule") ||
        !B.view("xt.cmap", pl.cmap, nr * 256, "one class map per rule") || !B.view("var.xt_off", off) ||
        !B.view("var.xt_ids", ids) || !B.view("xt.trans", pl.trans) || !B.view("xt.flags", pl.flags) ||
        !check_lists(off, ids, c.keys, 0xffff, nr,
                     {"var.xt_off", "var.xt_ids", "V*T+1 offsets", "a rule", "the rule table"}, bad))
        return false;
    static const char* size = "xt.desc holds an automaton of impossible size";
    for (size_t r = 0; r < nr; ++r) {
        const int32_t kind = x.xt_rule[4 * r], wb = x.xt_rule[4 * r + 1], wa = x.xt_rule[4 * r + 2];
        if (kind < 0 || kind >= XT_KINDS) return bad("xt.rule holds an unknown kind");
        if (wb < 0 || wa < 0) return bad("xt.rule holds a negative window");
        if (kind == XT_HOTWORD && wb == 0 && wa == 0) return bad("xt.rule holds a hotword rule without a window");
        if (!check_dfa(desc.sub(8 * r, 8), pl, {"xt.desc", "xt.trans", "xt.flags", "xt.cmap", size}, bad)) return false;
        add_dfa(x.xp, desc.sub(8 * r, 8), pl);
    }
    x.xtl = dedup_lists(off, ids);
    H.excl_text = true;
    return true;
}

// crypto_replace_ffx_fpe_config (rules with an FPE type): xf.fpe, per type key | alphabet << 16; xf.fpe_key,
// per key a record of XF_FPE_KEY_WORDS; xf.fpe_alpha, per alphabet a record of XF_FPE_ALPHA_WORDS (pii_layout.h).
// Everything ff1_apply indexes by is checked here: the kernels check nothing.
inline bool read_fpe(const Blob& B, HostXf& x, HostRules& H) {
    const Why& bad = B.bad;
    const size_t T = H.R.T;
    if (!B.has("xf.fpe") || !B.has("xf.fpe_key") || !B.has("xf.fpe_alpha")) return bad("FPE sections are not all present");
    if (!B.view("xf.fpe", x.fpe) || !B.view("xf.fpe_key", x.fpe_key) || !B.view("xf.fpe_alpha", x.fpe_alpha)) return false;
    if (x.fpe.n != T) return bad("xf.fpe does not hold one word per type");
    if (x.fpe_key.n == 0 || x.fpe_key.n % XF_FPE_KEY_WORDS != 0) return bad("xf.fpe_key does not hold whole key records");
    if (x.fpe_alpha.n == 0 || x.fpe_alpha.n % XF_FPE_ALPHA_WORDS != 0)
        return bad("xf.fpe_alpha does not hold whole alphabet records");
    const size_t nk = x.fpe_key.n / XF_FPE_KEY_WORDS, na = x.fpe_alpha.n / XF_FPE_ALPHA_WORDS;
    if (nk > (size_t)XF_FPE_KEYS_MAX) return bad("xf.fpe_key holds too many keys");
    for (size_t t = 0; t < T; ++t) {
        if (H.xf_kind[t] != PII_XF_FPE) continue;
        if ((x.fpe[t] & 0xffffu) >= nk) return bad("xf.fpe names a key past the key table");
        if ((x.fpe[t] >> 16) >= na) return bad("xf.fpe names an alphabet past the alphabet table");
    }
    for (size_t k = 0; k < nk; ++k) {
        const uint32_t nr = x.fpe_key[k * XF_FPE_KEY_WORDS];
        if (nr != 10 && nr != 12 && nr != 14) return bad("xf.fpe_key holds a round count that is not 10, 12 or 14");
    }
    for (size_t a = 0; a < na; ++a) {
        const View<uint32_t> rec = x.fpe_alpha.sub(a * XF_FPE_ALPHA_WORDS, XF_FPE_ALPHA_WORDS);
        const uint32_t radix = rec[0], nmin = rec[1], nmax = rec[2];
        const uint8_t* to_digit = reinterpret_cast<const uint8_t*>(rec.p + 4);
        const uint8_t *to_byte = to_digit + 128, *bv = to_byte + 96;
        if (radix < 2 || radix > 95) return bad("xf.fpe_alpha holds a radix outside 2..95");
        size_t inside = 0;
        for (uint32_t c = 0; c < 128; ++c) {
            if (to_digit[c] == 0xff) continue;
            if (to_digit[c] >= radix || to_byte[to_digit[c]] != c) return bad("xf.fpe_alpha holds maps that are not inverse");
            ++inside;
        }
        for (uint32_t d = 0; d < radix; ++d)
            if (to_byte[d] > 127 || to_digit[to_byte[d]] != d) return bad("xf.fpe_alpha holds maps that are not inverse");
        if (inside != radix) return bad("xf.fpe_alpha holds maps that are not inverse");
        if (nmin < 2 || nmin > nmax || nmax > (uint32_t)XF_FPE_NMAX) return bad("xf.fpe_alpha holds numeral limits out of range");
        for (int v = 0; v < 32; ++v)
            if (bv[v] == 0 || bv[v] > 16 || (v > 0 && bv[v] < bv[v - 1]))
                return bad("xf.fpe_alpha holds byte lengths that are not ascending up to 16");
    }
    H.fpe_nkeys = (uint32_t)nk;
    x.fpe_te0.resize(XF_FPE_TE0_WORDS);
    pii::fpe_te0(x.fpe_te0.data());
    return true;
}

// deidentify_config (without the sections every type is replaced by its "[NAME]" token) and the token
// tables behind the output
inline bool read_transformations(const Blob& B, HostXf& x, HostRules& H) {
    const Why& bad = B.bad;
    const size_t T = H.R.T;
    static const char* xf_bad = "transformation tables malformed";
    H.xf_kind.assign(T, (uint8_t)PII_XF_INFO_TYPE);
    x.maskp.assign(std::max<size_t>(T, 1) * XF_MASK_WORDS, 0u);
    View<uint8_t> kind, repl;
    View<uint32_t> ro, mask;
    if (B.has("xf.kind")) {
        if (!B.view("xf.kind", kind, T, "") || !B.view("xf.repl_off", ro, T + 1, "") || !B.view("xf.repl", repl) ||
            !B.view("xf.mask", mask, T * XF_MASK_WORDS, ""))
            return bad(xf_bad);
        for (size_t t = 0; t < T; ++t) {
            if (kind[t] > PII_XF_FPE || ro[t] > ro[t + 1] || ro[t + 1] > repl.n || ro[t + 1] - ro[t] > 255) return bad(xf_bad);
            H.xf_kind[t] = kind[t];
            H.xf_src |= kind[t] == PII_XF_MASK || kind[t] == PII_XF_KEEP || kind[t] == PII_XF_FPE;
            H.xf_mask |= kind[t] == PII_XF_MASK;
            H.xf_hash |= kind[t] == PII_XF_HASH;
            H.xf_fpe |= kind[t] == PII_XF_FPE;
        }
        if (H.xf_hash) {   // per type a key index, per key two midstates; a hash type's replacement is its placeholder
            if (!B.view("xf.hash_key", x.hash_key, T, "") || !B.view("xf.hash_mid", x.hash_mid) || x.hash_mid.n == 0 ||
                x.hash_mid.n % XF_HASH_KEY_WORDS != 0)
                return bad(xf_bad);
            for (size_t t = 0; t < T; ++t)
                if (H.xf_kind[t] == PII_XF_HASH &&
                    (x.hash_key[t] >= x.hash_mid.n / XF_HASH_KEY_WORDS || ro[t + 1] - ro[t] != XF_HASH_LEN))
                    return bad(xf_bad);
        }
        if (H.xf_fpe && !read_fpe(B, x, H)) return false;
        std::copy(mask.p, mask.p + mask.n, x.maskp.begin());
        for (size_t t = 0; t < T; ++t)
            if (H.xf_kind[t] == PII_XF_MASK && (x.maskp[t * XF_MASK_WORDS] & 0xffu) > 127u) return bad(xf_bad);
    }
    // tok_len: the per-type output length table behind out_len (T + 1 entries, as the offsets it replaces
    // in the k_select / k_win_select images)
    x.tok_off.assign(T + 1, 0);
    x.tok_len.assign(T + 1, 0);
    for (size_t t = 0; t < T; ++t) {
        if (H.xf_kind[t] == PII_XF_INFO_TYPE)
            x.tok += "[" + H.names[t] + "]";
        else if (H.xf_kind[t] == PII_XF_REPLACE || H.xf_kind[t] == PII_XF_HASH)   // (hash: the placeholder)
            x.tok.append(reinterpret_cast<const char*>(repl.p) + ro[t], ro[t + 1] - ro[t]);
        x.tok_off[t + 1] = (uint32_t)x.tok.size();
        const bool same_len = H.xf_kind[t] == PII_XF_MASK || H.xf_kind[t] == PII_XF_KEEP || H.xf_kind[t] == PII_XF_FPE;
        x.tok_len[t] = same_len ? XF_SAME_LEN : x.tok_off[t + 1] - x.tok_off[t];
    }
    x.tok += "\n";               // the re-scan window separator (k_win_redact piece source)
    H.R.nl_off = (uint32_t)x.tok.size() - 1;
    x.tok.append(32, '\0');     // k_redact reads aligned 16-byte windows past a token's end
    return true;
}

// SCAN groups >= 1: geometry, checked tables, the k_scan layout of each
inline bool read_scan_groups(const Blob& B, const CoreSecs& c, HostScan& s, HostRules& H) {
    const Why& bad = B.bad;
    const int64_t n_extra = c.meta[14];
    if (n_extra < 0 || n_extra + 1 > SCAN_GROUPS_MAX) return bad("too many SCAN groups");
    View<int64_t> gs;
    if (n_extra > 0 && (!B.has("scan.groups") || !B.view("scan.groups", gs) || gs.n < (size_t)n_extra * 4))
        return bad("SCAN group table missing");
    for (int64_t q = 1; q <= n_extra; ++q) {
        const View<int64_t> gm = gs.sub(4 * (q - 1), 4);
        const std::string nm = "scan.g" + std::to_string(q);
        View<uint8_t> cmap;
        View<uint16_t> trans, accid;
        if (!B.has(nm + ".cmap") || !B.has(nm + ".trans") || !B.has(nm + ".accid")) return bad("SCAN group tables malformed");
        if (!B.view(nm + ".cmap", cmap, 256, "one class per byte") || !B.view(nm + ".trans", trans) || !B.view(nm + ".accid", accid))
            return false;
        if (gm[0] < 1 || gm[0] > 65536 || gm[1] < 2 || gm[1] > 257) return bad("a SCAN group of impossible size");
        HostGroup h{};
        GroupTabs g;
        h.SD = (int)gm[0];
        h.CD = (int)gm[1];
        h.CDs = (h.CD + 1) & ~1;
        // a table past 64 KiB of LDS addresses is WIDE: rows padded to a multiple of 4 entries (8-byte
        // aligned), entries hold the row offset / 2, so 16-bit entries reach 128 KiB (and the u16
        // transition index of an event, 64k entries)
        if (SCAN_TD_BASE + (size_t)h.SD * h.CDs * 2 + 4 + SCAN_SPREAD_BYTES > 65536) {
            h.CDs = (h.CD + 3) & ~3;
            h.dsh = 1;
            if ((size_t)h.SD * h.CDs > 65536) return bad("a SCAN group exceeds 128 KiB of LDS");
        }
        const uint32_t tkb = SCAN_TD_BASE + (uint32_t)(h.SD * h.CDs) * 2;
        h.lds = tkb + 4 + SCAN_SPREAD_BYTES;                // + the K stub's row (2 entries), spread masks
        if (h.lds + FIX_LDS > 160 * 1024) return bad("a SCAN group exceeds the LDS");
        if (!check_scan(trans, accid, h.SD, h.CD, gm[2], H.R.n_dacc, [&](int b) { return cmap[b]; },
                        {nm + ".trans", nm + ".accid", nm + ".cmap", "SCAN group start state out of range"}, bad))
            return false;
        g.td.assign((size_t)h.SD * h.CDs, 0);
        g.dacc.assign((size_t)h.SD * h.CDs, 0);
        relayout(trans, accid, h.SD, h.CD, h.CDs, (int)gm[2], g.td.data(), g.dacc.data(), h.dsh);
        g.cmap4.resize(256);
        // class words of a group >= 1: the D half only (its K is the stub, stepped at tk_base)
        for (int b = 0; b < 256; ++b) g.cmap4[b] = SCAN_TD_BASE + 2u * cmap[b];
        H.groups.push_back(h);
        s.gt.push_back(std::move(g));
    }
    return true;
}

// the tables k_scan and the pair kernels read, derived from the checked D and K tables
inline void derive_scan_tables(const CoreSecs& c, HostScan& s, const RulesDev& R) {
    const size_t nd = (size_t)R.SD * R.CDs, nk = (size_t)R.SK * R.CKs;
    s.td.assign(nd, 0);
    s.dacc.assign(nd, 0);
    s.tk.assign(nk, 0);
    s.kacc.assign(nk, 0);
    relayout(c.d_trans, c.d_accid, R.SD, R.CD, R.CDs, c.d_start, s.td.data(), s.dacc.data());
    relayout(c.k_trans, c.k_accid, R.SK, R.CK, R.CKs, c.k_start, s.tk.data(), s.kacc.data());
    const uint32_t tk_base = SCAN_TD_BASE + (uint32_t)(nd / 2) * 4;
    s.cmap4.resize(256);
    for (int b = 0; b < 256; ++b)
        s.cmap4[b] = (SCAN_TD_BASE + 2u * (c.cmap2[b] & 0xffu)) | (tk_base + 2u * (uint32_t)(c.cmap2[b] >> 8)) << 16;
    for (size_t a = 0; a < R.n_kacc; ++a) {
        int m = KW_NONE;
        for (uint32_t i = c.k_acc_off[a]; i < c.k_acc_off[a + 1]; ++i) m = std::min<int>(m, c.k_acc_ids[i]);
        s.k_acc_min.push_back((uint16_t)m);
    }
    const View<uint32_t>& off = c.d_acc_off;
    s.d_npair.resize(nd);
    s.d_na.resize(nd);
    s.k_grp.resize(nk);
    for (size_t i = 0; i < nd; ++i) s.d_npair[i] = (uint16_t)(off[s.dacc[i] + 1] - off[s.dacc[i]]);
    for (size_t i = 0; i < nk; ++i) s.k_grp[i] = s.kacc[i] ? s.k_acc_min[s.kacc[i]] : (uint16_t)KW_NONE;
    for (auto& g : s.gt) {
        g.npair.resize(g.dacc.size());
        for (size_t i = 0; i < g.dacc.size(); ++i) g.npair[i] = (uint16_t)(off[g.dacc[i] + 1] - off[g.dacc[i]]);
    }
    for (size_t i = 0; i < nd; ++i) s.d_na[i] = s.d_npair[i] | (uint32_t)s.dacc[i] << 16;
}

// one buffer holding every table, 256-byte aligned sections (16 spare bytes after each)
inline void pack_rules(const CoreSecs& c, const HostExcl& x, const HostXf& xf, const HostScan& s, HostRules& H) {
    auto put = [&](std::pair<const void*, size_t> p) {
        const size_t o = (H.packed.size() + 255) & ~(size_t)255;
        H.packed.resize(o + p.second + 16, 0);
        if (p.second) std::memcpy(H.packed.data() + o, p.first, p.second);
        return o;
    };
    const std::pair<const void*, size_t> tabs[] = {
        part(s.cmap4), part(s.td), part(s.tk), part(s.dacc), part(c.d_acc_off), part(c.d_acc_ids), part(s.kacc),
        part(s.k_acc_min), part(s.d_npair), part(s.k_grp), part(s.d_na), part(c.det_type), part(c.det_val), part(c.det_lik),
        part(c.det_exidx), part(c.first_desc), part(c.hot_rule), part(c.hot_desc), part(c.var_enabled), part(c.var_minlik),
        part(c.rule_off), part(c.rule_ids), part(c.excl_off), part(c.excl_ids), part(xf.tok_off), part(xf.tok),
        part(xf.tok_len), part(H.xf_kind), part(xf.maskp)};
    static_assert(sizeof(tabs) / sizeof(tabs[0]) == TB_XF_MASK + 1, "one table per TB_* up to TB_XF_MASK, in that order");
    for (int i = 0; i <= TB_XF_MASK; ++i) H.off[i] = put(tabs[i]);
    static const uint16_t stub[2] = {0, 0};          // a group's K: one row, never accepting
    for (size_t q = 0; q < s.gt.size(); ++q) {
        size_t* o = H.groups[q].off;
        o[GT_CMAP4] = put(part(s.gt[q].cmap4));
        o[GT_TD] = put(part(s.gt[q].td));
        o[GT_TK] = put({stub, 4});
        o[GT_D_ACCID] = put(part(s.gt[q].dacc));
        o[GT_K_ACCID] = put({stub, 4});
        o[GT_D_NPAIR] = put(part(s.gt[q].npair));
    }
    if (H.xf_hash) {
        H.off[TB_HASH_KEY] = put(part(xf.hash_key));
        H.off[TB_HASH_MID] = put(part(xf.hash_mid));
    }
    if (H.excl_general) {
        H.off[TB_XG_OFF] = put(part(x.xg_off));
        H.off[TB_XG_IDS] = put(part(x.xg_ids));
        H.off[TB_XG_IDX] = put(part(x.xg_idx));
    }
    if (H.xf_fpe) {
        H.off[TB_FPE] = put(part(xf.fpe));
        H.off[TB_FPE_KEY] = put(part(xf.fpe_key));
        H.off[TB_FPE_ALPHA] = put(part(xf.fpe_alpha));
        H.off[TB_FPE_TE0] = put(part(xf.fpe_te0));
    }
}

// per-kernel LDS images: the full ones, k_excl_text's, the hot FIRST copy of an image past LDS, the
// list-less variants of a pair-kernel image past IMG_LDS_SPLIT
inline bool build_images(const Blob& B, const CoreSecs& c, const HostExcl& x, const HostXf& xf, const RuleKnobs& knobs,
                         HostRules& H) {
    const Why& bad = B.bad;
    const RulesDev& R = H.R;
    // absorbed match starts: the patterns' PRE states (absent in older blobs: nothing is dropped)
    View<int32_t> pre;
    if (B.has("det.first_pre")) {
        if (!B.view("det.first_pre", pre)) return false;
        if (pre.n < (size_t)R.P) return bad("det.first_pre is too short");
    }
    if (!knobs.first_drop) pre = {};
    auto fpre = [&](int p) { return pre.n ? pre[p] : -1; };
    for (int p = 0; p < R.P; ++p)
        if (fpre(p) >= c.first_desc[8 * p + 7]) return bad("det.first_pre names a state past its automaton");
    DfaPool fp, hp;
    for (int p = 0; p < R.P; ++p) add_dfa(fp, c.first_desc.sub(8 * p, 8), c.pool, fpre(p));
    for (int h = 0; h < R.n_hot; ++h) add_dfa(hp, c.hot_desc.sub(8 * h, 8), c.pool);
    if (hp.desc.empty()) hp.desc.assign(8, 0);
    const ListTab rl = dedup_lists(c.rule_off, c.rule_ids);
    const ListTab xl = dedup_lists(c.excl_off, c.excl_ids);
    const uint32_t aux = rl.w | xl.w << 3;
    H.lists_cl = rl.w != 0 || xl.w != 0;
    // per type: every hotword rule it has in any context variant (k_win_eval's resident bits)
    std::vector<uint32_t> thot(std::max(R.T, 1), 0u);
    for (int v = 0; v < R.V; ++v)
        for (int t = 0; t < R.T; ++t)
            for (uint32_t q = c.rule_off[v * R.T + t]; q < c.rule_off[v * R.T + t + 1]; ++q)
                if (c.rule_ids[q] < 32) thot[t] |= 1u << c.rule_ids[q];     // k_win_* cache the first WHOT_BITS
    ImageParts pf(FI_N), pe(EV_N), ps(SE_N), pw(WS_N);
    pf[FI_TRANS] = part(fp.trans);
    pf[FI_CMAP] = part(fp.cmap);
    pf[FI_DESC] = part(fp.desc);
    pe[EV_TRANS] = pw[WS_TRANS] = part(hp.trans);
    pe[EV_CMAP] = pw[WS_CMAP] = part(hp.cmap);
    pe[EV_HDESC] = pw[WS_HDESC] = part(hp.desc);
    pe[EV_HRULE] = pw[WS_HRULE] = part(c.hot_rule);
    pe[EV_DTYPE] = pw[WS_DTYPE] = ps[SE_DTYPE] = part(c.det_type);
    pe[EV_DVAL] = part(c.det_val);
    pe[EV_DLIK] = pw[WS_DLIK] = part(c.det_lik);
    pe[EV_ROFF] = pw[WS_ROFF] = part(rl.ix);
    pe[EV_RLOFF] = pw[WS_RLOFF] = part(rl.loff);
    pe[EV_RIDS] = pw[WS_RIDS] = part(rl.ids);
    pe[EV_THOT] = part(thot);
    pw[WS_VEN] = ps[SE_VEN] = part(c.var_enabled);
    pw[WS_VMIN] = ps[SE_VMIN] = part(c.var_minlik);
    pw[WS_DEX] = ps[SE_DEX] = part(c.det_exidx);
    pw[WS_XOFF] = ps[SE_XOFF] = part(xl.ix);
    pw[WS_XLOFF] = ps[SE_XLOFF] = part(xl.loff);
    pw[WS_XIDS] = ps[SE_XIDS] = part(xl.ids);
    pw[WS_TOKOFF] = ps[SE_TOKOFF] = part(xf.tok_len);
    static const char* img_bad = "rule table upload failed";
    if (!pack_image(pw, aux, H.img_wsel) || !pack_image(pf, 0, H.img_first) || !pack_image(pe, aux, H.img_eval) ||
        !pack_image(ps, aux, H.img_sel))
        return bad(img_bad);
    if (H.excl_text) {
        ImageParts px(TX_N);
        px[TX_TRANS] = part(x.xp.trans);
        px[TX_CMAP] = part(x.xp.cmap);
        px[TX_DESC] = part(x.xp.desc);
        px[TX_RULE] = part(x.xt_rule);
        px[TX_DTYPE] = part(c.det_type);
        px[TX_OFF] = part(x.xtl.ix);
        px[TX_IDS] = part(x.xtl.ids);
        px[TX_LOFF] = part(x.xtl.loff);
        if (!pack_image(px, x.xtl.w, H.img_xtext)) return bad(img_bad);
    }
    if (H.img_first.global) {
        DfaPool hf;
        const uint32_t ph = pack_first_hot(knobs, R.P, c.first_desc, c.pool, fpre, hf);
        if (ph > 0) {
            ImageParts parts(FI_N);
            parts[FI_TRANS] = part(hf.trans);
            parts[FI_CMAP] = part(hf.cmap);
            parts[FI_DESC] = part(hf.desc);
            if (!pack_image(parts, 0, H.img_first_hot)) return bad(img_bad);
            H.first_p_hot = ph;
        }
    }
    // the list-less variants of a pair-kernel image past IMG_LDS_SPLIT (the kernel reads the lists from
    // L2): kept only when they fit where the full image did not
    if (H.img_eval.li.total > IMG_LDS_SPLIT) {
        pe[EV_ROFF] = pe[EV_RLOFF] = pe[EV_RIDS] = {nullptr, 0};
        if (!pack_image(pe, 0, H.img_eval_rg)) return bad(img_bad);
        if (H.img_eval_rg.global) H.img_eval_rg = HostImage{};
    }
    if (H.img_sel.li.total > IMG_LDS_SPLIT) {
        ps[SE_XOFF] = ps[SE_XLOFF] = ps[SE_XIDS] = {nullptr, 0};
        if (!pack_image(ps, 0, H.img_sel_rg)) return bad(img_bad);
        if (H.img_sel_rg.global || H.img_sel_rg.li.total > 64 * 1024) H.img_sel_rg = HostImage{};   // (no gain: keep the full image)
    }
    H.scan_lds = SCAN_TD_BASE + (size_t)(R.SD * R.CDs / 2) * 4 + (size_t)(R.SK * R.CKs / 2) * 4 + SCAN_SPREAD_BYTES;
    if (H.scan_lds > 160 * 1024) return bad("SCAN tables do not fit in LDS");
    return true;
}

// Returns nullptr and fills `H`, or the first defect of the blob.
inline const char* build_host_rules(const uint8_t* blob, size_t n, const RuleKnobs& knobs, HostRules& H) {
    Blob B{{}, Why{H.defect}};
    if (!parse_blob(blob, n, B.secs)) return "not a rules blob";
    CoreSecs c;
    HostExcl x;
    HostXf xf;
    HostScan s;
    if (!read_core(B, c, H) || !read_general_exclusion(B, c, x, H) || !read_text_exclusion(B, c, x, H) ||
        !read_transformations(B, xf, H) || !read_scan_groups(B, c, s, H))
        return H.defect.c_str();
    derive_scan_tables(c, s, H.R);
    pack_rules(c, x, xf, s, H);
    return build_images(B, c, x, xf, knobs, H) ? nullptr : H.defect.c_str();
}

}  // namespace
