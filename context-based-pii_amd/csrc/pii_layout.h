// pii_layout.h - table and LDS-image layout shared by the kernels (pii_engine.hip, pii_device.h) and
// the host-side rule preparation (pii_rules_host.h).  Plain C++: no HIP header, no device code.
//
// Everything but DFA_STATE_MASK sits in an unnamed namespace, as it did in the kernel file: RulesDev and
// LdsImage are kernel parameter types, and the kernels' symbol names carry their namespace.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pii {
// In the kernels' LDS images every transition entry is  next_state | flags(next_state) << 14
// (see the DFA runners of pii_device.h)
constexpr uint32_t DFA_STATE_MASK = 0x3fffu;
}  // namespace pii

namespace {

constexpr int NE_MAX = 2;          // excluder patterns
constexpr int NX_MAX = 64;         // excluder patterns of a GENERAL rule set (k_exclude; compiler.py mirrors both)
constexpr uint16_t XG_PARTIAL = 0x8000;   // general exclusion list entry: excluder type | this bit for PARTIAL_MATCH
constexpr int KW_NONE = 0x7fff;
// text exclusion rules (k_excl_text; compiler.py XT_*): xt.rule entry = (kind, window_before, window_after, 0).
// The rule's HOT-form automaton is run over the candidate's own bytes -- SEARCH: an accept drops it; FULL /
// INVERSE (the automaton of \A(?:pattern)\Z): an accept / no accept drops it -- or, HOTWORD, over the
// proximity windows around it, clipped to the row: an accept in either drops it.
enum { XT_SEARCH = 0, XT_FULL = 1, XT_INVERSE = 2, XT_HOTWORD = 3, XT_KINDS = 4 };

struct RulesDev {
    int P, G, T, V, SD, CD, d_start, SK, CK, k_start, n_hot, min_len;
    int kw_always_min, NE;
    int CDs, CKs;                // row strides of the SCAN tables (CD / CK rounded up to even; a WIDE
                                 // group's D: to a multiple of 4)
    int dsh;                     // D entry = row byte offset >> dsh (| flags): 0, or 1 for a WIDE SCAN
                                 // group >= 1 (D table up to 128 KiB; its class words carry no K half)
    uint32_t n_dacc, n_kacc;     // D / K accept sets
    const uint32_t* cmap4;    // [256] 2*classD | 2*classK << 16 (byte offsets)
    const uint16_t* td;       // [SD*CDs] LDS byte address of the next row in k_scan | accept (bit 0)
                              //   | the next row's end-of-text transition accepts (bit 1)
    const uint16_t* tk;       // [SK*CKs]
    const uint16_t* d_accid;  // [SD*CDs]
    const uint32_t* d_na;     // [SD*CDs] d_npair | d_accid << 16 (the pair write pass: one gather for both)
    const uint32_t* d_acc_off;
    const uint16_t* d_acc_ids;
    const uint16_t* k_accid;  // [SK*CKs]
    const uint16_t* k_acc_min;  // per K accept set: smallest context group
    const uint16_t* d_npair;    // [SD*CDs] per D transition: pairs of its accept set (k_pairs count pass)
    const uint16_t* k_grp;      // [SK*CKs] per K transition: smallest context group it accepts, or KW_NONE
    const uint16_t* det_type;
    const uint8_t* det_val;
    const uint8_t* det_lik;
    const uint8_t* det_exidx;   // excluder slot or 0xff
    const int32_t* first_desc;  // [P*8]
    const int32_t* hot_rule;    // [n_hot*4] wb, wa, fixed, rel
    const int32_t* hot_desc;    // [n_hot*8]
    const uint8_t* var_enabled;  // [V*T]
    const uint8_t* var_minlik;   // [V]
    const uint32_t* rule_off;    // [V*T+1]
    const uint16_t* rule_ids;
    const uint32_t* excl_off;    // [V*T+1]
    const uint16_t* excl_ids;
    const uint32_t* tok_off;     // [T+1] into tok_bytes: a type's fixed output ("[NAME]", its replace_config
                                 // string, a hash type's 44-byte placeholder, nothing for redact_config / mask /
                                 // keep)
    const uint8_t* tok_bytes;
    const uint32_t* tok_len;     // [T+1] per type: its fixed output length, or XF_SAME_LEN (mask / keep); see out_len
    const uint8_t* xf_kind;      // [T] PII_XF_*
    const uint32_t* xf_mask;     // [T*XF_MASK_WORDS] mask types: char | reverse << 8, number_to_mask, 128-bit skip set
    uint32_t nl_off;             // tok_bytes[nl_off] = '\n' (the re-scan window separator)
};

constexpr uint32_t XF_SAME_LEN = 0x80000000u;
constexpr int XF_MASK_WORDS = 8;
constexpr int XF_HASH_KEY_WORDS = 16;
constexpr uint32_t XF_HASH_LEN = 44;      // base64 of a SHA-256 digest
// crypto_replace_ffx_fpe_config (pii_fpe.h).  A key record: Nr, the 4 * (Nr + 1) AES round-key words, zeros.
// An alphabet record: radix, nmin, nmax, 0; the byte -> digit map [128] (0xff: outside the alphabet); the
// digit -> byte map [96]; b(v), v = 1 .. 32, the bytes of radix^v - 1.  Per type: key | alphabet << 16.
constexpr int XF_FPE_KEY_WORDS = 64;
constexpr int XF_FPE_ALPHA_WORDS = 68;
constexpr int XF_FPE_NMAX = 64;           // numerals at most (v <= 32, NUM(B) <= 16 bytes)
constexpr int XF_FPE_KEYS_MAX = 16;       // distinct keys of one rule set (k_fpe keeps their round keys in LDS)
constexpr int XF_FPE_TE0_WORDS = 256;     // the AES round table fpe_te0 builds (beside the keys in the rules buffer)

// k_scan's table entries are absolute LDS byte addresses of the next row, bit 0 = accept (scan_tables);
// k_scan has no static LDS, so its dynamic region starts at LDS address 0 and an entry IS the address
constexpr uint32_t SCAN_TD_BASE = 1024;     // after the 256-entry class map
constexpr uint32_t SCAN_SPREAD_BYTES = 512; // k_scan's 256 group masks (scan_spread), after the K table

constexpr int FIX_Q = 512;
// k_scan_fix's LDS past the scan tables (the tables' entries are absolute LDS addresses, so the kernel
// declares no static LDS): queue, entry states, previous round's lanes, counters
constexpr size_t FIX_LDS = (3 * FIX_Q + 4) * 4;

constexpr int SCAN_GROUPS_MAX = 8;

// LDS images of rule tables, one per kernel (only what that kernel reads, so the pair kernels keep
// two 1024-thread workgroups per CU).  Sections are 16-byte aligned; off[] are byte offsets.
constexpr int IMG_MAX = 16;
struct LdsImage {
    uint32_t off[IMG_MAX];
    uint32_t total;    // bytes, multiple of 16
    uint32_t aux;      // index widths of the image's list tables (list_range): rule lists | exclusion lists << 3
};
enum { FI_TRANS, FI_CMAP, FI_DESC, FI_N };
enum { EV_TRANS, EV_CMAP, EV_HDESC, EV_HRULE, EV_DTYPE, EV_DVAL, EV_DLIK, EV_ROFF, EV_RIDS, EV_THOT, EV_RLOFF, EV_N };
// k_win_select: everything k_select reads + the HOT automata and the variants' hotword rule lists
enum { WS_TRANS, WS_CMAP, WS_HDESC, WS_HRULE, WS_DTYPE, WS_DLIK, WS_VEN, WS_VMIN, WS_DEX, WS_XOFF, WS_XIDS,
       WS_TOKOFF, WS_ROFF, WS_RIDS, WS_RLOFF, WS_XLOFF, WS_N };
enum { SE_DTYPE, SE_VEN, SE_VMIN, SE_DEX, SE_XOFF, SE_XIDS, SE_TOKOFF, SE_XLOFF, SE_N };
// k_excl_text: the text exclusion rules' automata, the rules, their per-(variant, type) lists (aux = the
// lists' index width, list_range), the patterns' types
enum { TX_TRANS, TX_CMAP, TX_DESC, TX_RULE, TX_DTYPE, TX_OFF, TX_IDS, TX_LOFF, TX_N };

constexpr size_t IMG_LDS_MAX = 160 * 1024;
// k_pair_first<true>'s LDS copy: most of the LDS, one 1024-thread workgroup per CU (config 5: 40 / 78 /
// 156 KB -> 999 / 934 / 885 us: more automata in LDS beat two workgroups per CU)
constexpr size_t FIRST_HOT_LDS = 156 * 1024;
constexpr size_t FIRST_HOT_BIG = 8 * 1024;      // ... which skips automata larger than this (prefix of
                                                // ids, 78 KB: 982 -> 933 us)
constexpr size_t IMG_LDS_SPLIT = 80 * 1024;    // pair-kernel image size past which its per-(variant, type) lists stay in L2

}  // namespace
