// crypto_replace_ffx_fpe_config: FF1 (NIST SP 800-38G) over AES (FIPS-197) under an empty tweak.  One body,
// ff1_apply, for the batch post-pass (k_fpe), the window post-pass (k_win_fpe) and, in its decrypt form
// ff1_apply<true>, pii_reidentify (k_reid); the kernels only locate their finding and stage the tables.  It is written in plain C++ with every table behind a pointer
// and no device builtin, so the same text compiles for the host: tests/fpe_body_main.cpp runs it on the CPU
// under the sanitizers.  In the kernels te0, the key record and the numerals live in LDS, the alphabet record
// in the rules buffer.  Nothing here is indexed at run time but those tables: the cipher state, the limbs of
// NUM(B) and of y are scalars, so the kernels need no scratch memory.
#pragma once

#include <cstdint>

#include "pii_layout.h"

#if defined(__HIPCC__)
#define PII_FPE_FN __host__ __device__ __forceinline__
#else
#define PII_FPE_FN inline
#endif

namespace pii {

// The one AES table: te0[x] = (02.S[x], S[x], S[x], 03.S[x]), most significant byte first.  The other three
// columns of MixColumns are its rotations, the last round's S[x] is its second byte.  S is generated as
// FIPS-197 5.1.1 defines it: the inverse in GF(2^8), then the affine transformation.  (host only: the rules
// buffer carries the table to the kernels)
inline void fpe_te0(uint32_t* te0) {
    uint8_t box[256];
    uint8_t p = 1, q = 1;
    do {
        p = (uint8_t)(p ^ (p << 1) ^ ((p & 0x80) ? 0x1B : 0));      // p *= 3
        q ^= (uint8_t)(q << 1);                                     // q /= 3
        q ^= (uint8_t)(q << 2);
        q ^= (uint8_t)(q << 4);
        if (q & 0x80) q ^= 0x09;
        const uint8_t x = (uint8_t)(q ^ (q << 1 | q >> 7) ^ (q << 2 | q >> 6) ^ (q << 3 | q >> 5) ^ (q << 4 | q >> 4));
        box[p] = x ^ 0x63;
    } while (p != 1);
    box[0] = 0x63;
    for (int i = 0; i < 256; ++i) {
        const uint32_t s = box[i], s2 = ((s << 1) ^ ((s & 0x80u) ? 0x11Bu : 0u)) & 0xffu;
        te0[i] = s2 << 24 | s << 16 | s << 8 | (s2 ^ s);
    }
}

PII_FPE_FN uint32_t fpe_ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// One block, in place: s0 .. s3 are its four big-endian words.  key: Nr, then the round keys.
PII_FPE_FN void aes_encrypt(const uint32_t* te0, const uint32_t* key, uint32_t& s0, uint32_t& s1, uint32_t& s2,
                            uint32_t& s3) {
    const int nr = (int)key[0];
    const uint32_t* rk = key + 1;
    s0 ^= rk[0], s1 ^= rk[1], s2 ^= rk[2], s3 ^= rk[3];
    for (int r = 1; r < nr; ++r) {
        rk += 4;
        const uint32_t t0 = te0[s0 >> 24] ^ fpe_ror(te0[(s1 >> 16) & 255u], 8) ^ fpe_ror(te0[(s2 >> 8) & 255u], 16) ^
                            fpe_ror(te0[s3 & 255u], 24) ^ rk[0];
        const uint32_t t1 = te0[s1 >> 24] ^ fpe_ror(te0[(s2 >> 16) & 255u], 8) ^ fpe_ror(te0[(s3 >> 8) & 255u], 16) ^
                            fpe_ror(te0[s0 & 255u], 24) ^ rk[1];
        const uint32_t t2 = te0[s2 >> 24] ^ fpe_ror(te0[(s3 >> 16) & 255u], 8) ^ fpe_ror(te0[(s0 >> 8) & 255u], 16) ^
                            fpe_ror(te0[s1 & 255u], 24) ^ rk[2];
        const uint32_t t3 = te0[s3 >> 24] ^ fpe_ror(te0[(s0 >> 16) & 255u], 8) ^ fpe_ror(te0[(s1 >> 8) & 255u], 16) ^
                            fpe_ror(te0[s2 & 255u], 24) ^ rk[3];
        s0 = t0, s1 = t1, s2 = t2, s3 = t3;
    }
    rk += 4;
    auto sb = [te0](uint32_t x) { return (te0[x] >> 8) & 255u; };
    const uint32_t t0 = (sb(s0 >> 24) << 24 | sb((s1 >> 16) & 255u) << 16 | sb((s2 >> 8) & 255u) << 8 | sb(s3 & 255u)) ^ rk[0];
    const uint32_t t1 = (sb(s1 >> 24) << 24 | sb((s2 >> 16) & 255u) << 16 | sb((s3 >> 8) & 255u) << 8 | sb(s0 & 255u)) ^ rk[1];
    const uint32_t t2 = (sb(s2 >> 24) << 24 | sb((s3 >> 16) & 255u) << 16 | sb((s0 >> 8) & 255u) << 8 | sb(s1 & 255u)) ^ rk[2];
    const uint32_t t3 = (sb(s3 >> 24) << 24 | sb((s0 >> 16) & 255u) << 16 | sb((s1 >> 8) & 255u) << 8 | sb(s2 & 255u)) ^ rk[3];
    s0 = t0, s1 = t1, s2 = t2, s3 = t3;
}

// One limb of a short division by r < 2^7, as two 16-bit steps: w = (rem : w) / r, rem = the remainder.
// A step's dividend is below r * 2^16 < 2^23, where the multiplication by mul = ceil(2^32 / r) gives the exact
// quotient (the error term is below 2^23 / 2^32, a fractional part is at most 1 - 1 / r).
PII_FPE_FN void fpe_div(uint32_t& w, uint32_t& rem, uint32_t r, uint32_t mul) {
    uint32_t cur = rem << 16 | w >> 16;
    const uint32_t qh = (uint32_t)(((uint64_t)cur * mul) >> 32);
    rem = cur - qh * r;
    cur = rem << 16 | (w & 0xffffu);
    const uint32_t ql = (uint32_t)(((uint64_t)cur * mul) >> 32);
    rem = cur - ql * r;
    w = qh << 16 | ql;
}

// The finding in[0, len) has been copied to o[0, len) unchanged.  Its bytes of the alphabet, in order, are the
// numeral string X of n numerals; FF1 encrypts it and the ciphertext numerals' characters are written to the
// same positions of o.  Every other byte stays.  With n < nmin or n > nmax nothing is encrypted: o[0, len)
// becomes '*'.  Only o[0, len) is written.  num: this caller's XF_FPE_NMAX numerals, numeral i at num[i * stride].
//
// FF1 under the empty tweak (SP 800-38G, Algorithm 7, t = 0): u = n / 2, v = n - u, b = b(v) <= 16 bytes,
// d = 4 * ceil(b / 4) + 4 <= 20.  P is one block and the same in every round: its AES is taken once.  Q is the
// round number and NUM(B) in b bytes: one block for b <= 15, two for b = 16.  S, the first d bytes, needs a
// second block only for d = 20.  A lies in num[0, u) and B after it; a round writes C over A and the two
// change roles, so after the ten rounds X stands in place.  c = (NUM(A) + y) mod radix^m needs no modulus:
// y mod radix^m is y's low m digits, m short divisions of y's five limbs, each added to A's numeral with the
// carry; the carry out of the top numeral is dropped.
//
// DEC: the inverse (Algorithm 8), called with in == o (in[i] is read before o[i] is written).  The rounds run
// i = 9 .. 0; round i's A-slot and B-slot are the ones encryption round i used, so the A-slot holds what that
// round wrote, y comes from the B-slot as above, and the A-slot becomes (A - y mod radix^m) mod radix^m: the
// same remainders, subtracted with a borrow that is dropped out of the top numeral.  With n out of range the
// decrypt form writes nothing: a fail-closed "***" stays "***", a re-identify never destroys text.
template <bool DEC = false>
PII_FPE_FN void ff1_apply(const uint32_t* te0, const uint32_t* key, const uint32_t* alpha, const uint8_t* in,
                          const int len, uint8_t* o, uint8_t* num, const int stride) {
    const uint32_t radix = alpha[0], nmin = alpha[1], nmax = alpha[2];
    const uint8_t* to_digit = reinterpret_cast<const uint8_t*>(alpha + 4);
    const uint8_t* to_byte = to_digit + 128;
    const uint8_t* bv = to_byte + 96;
    uint32_t n = 0;
    for (int i = 0; i < len; ++i) {
        const uint32_t c = in[i];
        if (c < 128u && to_digit[c] != 0xffu) {
            if (n < nmax) num[n * stride] = to_digit[c];
            ++n;
        }
    }
    if (n < nmin || n > nmax) {
        if (!DEC)
            for (int i = 0; i < len; ++i) o[i] = '*';
        return;
    }
    const uint32_t u = n >> 1, v = n - u;
    const uint32_t b = bv[v - 1], dw = ((b + 3) >> 2) + 1;          // d = 4 * dw
    const uint32_t mul = 0xffffffffu / radix + 1u;
    uint32_t p0 = 0x01020100u, p1 = radix << 16 | 10u << 8 | (u & 255u), p2 = n, p3 = 0;
    aes_encrypt(te0, key, p0, p1, p2, p3);
    for (uint32_t rnd = 0; rnd < 10; ++rnd) {
        const uint32_t i = DEC ? 9u - rnd : rnd;
        const bool even = (i & 1u) == 0;
        const uint32_t a0 = even ? 0 : u, m = even ? u : v;         // A = num[a0, a0 + m)
        const uint32_t b0 = even ? u : 0, bl = even ? v : u;        // B = num[b0, b0 + bl)
        uint32_t l0 = 0, l1 = 0, l2 = 0, l3 = 0;                    // NUM(B), least significant limb first
        for (uint32_t k = 0; k < bl; ++k) {
            uint64_t t = (uint64_t)l0 * radix + num[(b0 + k) * stride];
            l0 = (uint32_t)t;
            t = (uint64_t)l1 * radix + (t >> 32);
            l1 = (uint32_t)t;
            t = (uint64_t)l2 * radix + (t >> 32);
            l2 = (uint32_t)t;
            t = (uint64_t)l3 * radix + (t >> 32);
            l3 = (uint32_t)t;
        }
        uint32_t s0 = p0, s1 = p1, s2 = p2, s3 = p3;
        if (b < 16u) {                                              // Q = zeros, i, NUM(B) in b bytes
            const uint32_t ib = i << (8u * (b & 3u)), il = b >> 2;
            s0 ^= l3 | (il == 3u ? ib : 0u);
            s1 ^= l2 | (il == 2u ? ib : 0u);
            s2 ^= l1 | (il == 1u ? ib : 0u);
            s3 ^= l0 | (il == 0u ? ib : 0u);
            aes_encrypt(te0, key, s0, s1, s2, s3);
        } else {                                                    // 15 zeros and i, then NUM(B)
            s3 ^= i;
            aes_encrypt(te0, key, s0, s1, s2, s3);
            s0 ^= l3, s1 ^= l2, s2 ^= l1, s3 ^= l0;
            aes_encrypt(te0, key, s0, s1, s2, s3);
        }
        uint32_t y4, y3, y2, y1, y0;                                // y = the first 4 * dw bytes of S
        if (dw == 5u) {
            uint32_t e0 = s0, e1 = s1, e2 = s2, e3 = s3 ^ 1u;
            aes_encrypt(te0, key, e0, e1, e2, e3);
            y4 = s0, y3 = s1, y2 = s2, y1 = s3, y0 = e0;
        } else if (dw == 4u) {
            y4 = 0, y3 = s0, y2 = s1, y1 = s2, y0 = s3;
        } else if (dw == 3u) {
            y4 = 0, y3 = 0, y2 = s0, y1 = s1, y0 = s2;
        } else {
            y4 = 0, y3 = 0, y2 = 0, y1 = s0, y0 = s1;
        }
        uint32_t carry = 0;
        for (uint32_t k = 0; k < m; ++k) {
            uint32_t rem = 0;
            fpe_div(y4, rem, radix, mul);
            fpe_div(y3, rem, radix, mul);
            fpe_div(y2, rem, radix, mul);
            fpe_div(y1, rem, radix, mul);
            fpe_div(y0, rem, radix, mul);
            uint8_t* a = num + (a0 + m - 1u - k) * stride;
            if (DEC) {
                const int32_t s = (int32_t)*a - (int32_t)rem - (int32_t)carry;      // carry: the borrow
                carry = s < 0 ? 1u : 0u;
                *a = (uint8_t)(s + (carry ? (int32_t)radix : 0));
            } else {
                uint32_t s = *a + rem + carry;
                carry = s >= radix ? 1u : 0u;
                s -= carry ? radix : 0u;
                *a = (uint8_t)s;
            }
        }
    }
    uint32_t k = 0;
    for (int i = 0; i < len; ++i) {
        const uint32_t c = in[i];
        if (c < 128u && to_digit[c] != 0xffu) o[i] = to_byte[num[k++ * stride]];
    }
}

}  // namespace pii
