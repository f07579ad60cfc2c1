// The transformations that compute a finding's output from its bytes, character_mask_config (mask_walk) and
// crypto_hash_config (hmac_b64): one body each for the batch post-passes (k_mask, k_hash) and the window
// post-passes (k_win_mask, k_win_hash), which only locate their finding (input, output, type, length).
#pragma once

#include "pii_device.h"

namespace pii {

// ------------------------------------------------------------------------------ character_mask_config
// The code-point state machine, one byte per step: b = the byte at o[i], newcp = it starts a code point.
// There the decision for the whole code point is taken: an ASCII byte of the skip set is kept and not
// counted, anything else is masked.  False: number_to_mask code points are masked, the walk ends.
__device__ __forceinline__ bool mask_step(const uint4& m0, const uint2& m1, uint8_t mc, uint32_t limit,
                                          uint32_t& masked, bool& cur, uint8_t* o, uint32_t b, int i, bool newcp) {
    if (newcp) {
        if (masked >= limit) return false;
        const uint32_t sw = b < 32u ? m0.z : b < 64u ? m0.w : b < 96u ? m1.x : m1.y;
        cur = !(b < 128u && ((sw >> (b & 31u)) & 1u));
        masked += cur ? 1u : 0u;
    }
    if (cur) o[i] = mc;
    return true;
}

// The finding in[0, len) has been copied to o[0, len) unchanged; m0, m1 are its type's XF_MASK_WORDS words
// (character | reverse_order << 8, number_to_mask, the 128-bit skip set).  Walks the finding's UTF-8 code
// points (from the end when reverse_order) and overwrites every byte of a masked one with the masking
// character, until number_to_mask code points are masked (0 = all); only o[0, len) is written.  A per-byte
// state machine, so that the text is read as 16-byte windows (load16: only aligned chunks that hold a byte
// of the finding) instead of one dependent byte load per step.  A code point starts at a byte that is not a
// continuation byte (10xxxxxx); walking backwards, at the byte after a start.  The mask words by value:
// held by reference, the compiler keeps them in scratch memory and indexes the skip set there.
__device__ __forceinline__ void mask_walk(const uint4 m0, const uint2 m1, const uint8_t* in, uint8_t* o,
                                          const int len) {
    const uint8_t mc = (uint8_t)(m0.x & 0xffu);
    const bool rev = ((m0.x >> 8) & 1u) != 0;
    const uint32_t limit = m0.y ? m0.y : 0xffffffffu;
    uint32_t masked = 0;
    bool cur = false;                            // the code point being walked is masked
    auto step = [&](uint32_t b, int i, bool newcp) -> bool {
        return mask_step(m0, m1, mc, limit, masked, cur, o, b, i, newcp);
    };
    if (!rev) {
        for (int j = 0; j < len; j += 16) {
            const int n = len - j < 16 ? len - j : 16;
            uint4 w = load16(in + j, 0, n);
            for (int k = 0; k < n; ++k) {
                const uint32_t b = w.x & 0xffu;
                if (!step(b, j + k, (b & 0xC0u) != 0x80u || j + k == 0)) return;
                shr8(w);
            }
        }
    } else {
        bool newcp = true;                       // the byte after this one starts a code point (or is the end)
        for (int j = len; j > 0; j -= 16) {
            const int w0 = j - 16, klo = w0 < 0 ? -w0 : 0;      // window [w0, j), its bytes klo .. 15 in the span
            uint4 w = load16(in + w0, klo, 16);
            for (int k = 15; k >= klo; --k) {
                const uint32_t b = w.w >> 24;
                if (!step(b, w0 + k, newcp)) return;
                newcp = (b & 0xC0u) != 0x80u;
                w.w = (w.w << 8) | (w.z >> 24);
                w.z = (w.z << 8) | (w.y >> 24);
                w.y = (w.y << 8) | (w.x >> 24);
                w.x <<= 8;
            }
        }
    }
}

// ---------------------------------------------------------------------------------- crypto_hash_config
// SHA-256 (FIPS 180-4) on the vector ALUs.  One compression keeps the message schedule as a rolling
// 16-word window and unrolls the 64 rounds, so every array index is a compile-time constant and the
// state, the window and the round constants (literals) stay in registers: no scratch.
__device__ __forceinline__ uint32_t sha_rotr(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }

__device__ __forceinline__ void sha256_compress(uint32_t (&h)[8], uint32_t (&w)[16]) {
    constexpr uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
        0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
        0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
        0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
        0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
        0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        if (i >= 16) {
            const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            w[i & 15] += (sha_rotr(w15, 7) ^ sha_rotr(w15, 18) ^ (w15 >> 3)) + w[(i + 9) & 15] +
                         (sha_rotr(w2, 17) ^ sha_rotr(w2, 19) ^ (w2 >> 10));
        }
        const uint32_t t1 = hh + (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) + (g ^ (e & (f ^ g))) + K[i] +
                            w[i & 15];
        const uint32_t t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) + ((a & b) | (c & (a | b)));
        hh = g;
        g = f;
        f = e;
        e = d + t1;
        d = c;
        c = b;
        b = a;
        a = t1 + t2;
    }
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
    h[4] += e;
    h[5] += f;
    h[6] += g;
    h[7] += hh;
}

// character c (0..42) of the base64 of the 256-bit digest d[0..7] (d[8] = 0: the last character's low bits)
template <int C>
__device__ __forceinline__ uint8_t b64_char(const uint32_t (&d)[9]) {
    constexpr int p = 6 * C, wi = p >> 5, o = p & 31;
    uint32_t v;
    if constexpr (o <= 26) v = d[wi] >> (26 - o);
    else v = (d[wi] << (o - 26)) | (d[wi + 1] >> (58 - o));
    v &= 63u;
    uint32_t ch = v + 65u;                  // A-Z
    ch += v >= 26u ? 6u : 0u;               // a-z
    ch -= v >= 52u ? 75u : 0u;              // 0-9
    ch -= v >= 62u ? 15u : 0u;              // +
    ch += v == 63u ? 3u : 0u;               // /
    return (uint8_t)ch;
}
template <int C>
__device__ __forceinline__ void b64_store(const uint32_t (&d)[9], uint8_t* o) {
    if constexpr (C < 43) {
        o[C] = b64_char<C>(d);
        b64_store<C + 1>(d, o);
    }
}

// Writes base64(HMAC-SHA256(key, in[0, len))) to o[0, 44), over the type's 44-byte placeholder and nothing
// else.  The rules carry the key as its two midstates, mid[0..7] and mid[8..15] (the SHA-256 state after the
// key ^ ipad and the key ^ opad block), so the inner hash continues from the first over the finding's bytes
// (total length 64 + len) and the outer from the second over the 32-byte inner digest (total length 96):
// ceil((len + 9) / 64) + 1 compressions.  The text is read as 16-byte windows (load16, as in mask_walk).
__device__ __forceinline__ void hmac_b64(const uint32_t* __restrict__ mid, const uint8_t* in, const int len,
                                         uint8_t* o) {
    uint32_t h[8], w[16];
    {
        const uint4 m0 = *reinterpret_cast<const uint4*>(mid), m1 = *reinterpret_cast<const uint4*>(mid + 4);
        h[0] = m0.x, h[1] = m0.y, h[2] = m0.z, h[3] = m0.w, h[4] = m1.x, h[5] = m1.y, h[6] = m1.z, h[7] = m1.w;
    }
    // inner hash: the data blocks, 0x80 after the last byte, zeros, and the bit length in the last two
    // words of the first block with room for it (rem <= 55, rem = bytes left at the block's start; < 0 in
    // a block that holds only padding)
    for (int base = 0;; base += 64) {
        const int rem = len - base;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = rem - 16 * q;                    // finding bytes from this window's start
            uint4 v = make_uint4(0, 0, 0, 0);
            if (n > 0) v = load16(in + base + 16 * q, 0, n < 16 ? n : 16);
            const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int m = n - 4 * k;                   // ... from this word's start
                uint32_t u = x[k] & bytemask(m);
                if (m >= 0 && m < 4) u |= 0x80u << (8 * m);
                w[4 * q + k] = __builtin_bswap32(u);
            }
        }
        const bool last = rem <= 55;
        if (last) {
            w[14] = 0;                                     // (len < 2^29: the length fits the low word)
            w[15] = (64u + (uint32_t)len) * 8u;
        }
        sha256_compress(h, w);
        if (last) break;
    }
    // outer hash: the inner digest, padded to one block, total length 64 + 32 bytes
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = h[i];
    w[8] = 0x80000000u;
#pragma unroll
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = 96u * 8u;
    {
        const uint4 m0 = *reinterpret_cast<const uint4*>(mid + 8), m1 = *reinterpret_cast<const uint4*>(mid + 12);
        h[0] = m0.x, h[1] = m0.y, h[2] = m0.z, h[3] = m0.w, h[4] = m1.x, h[5] = m1.y, h[6] = m1.z, h[7] = m1.w;
    }
    sha256_compress(h, w);
    const uint32_t d[9] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], 0u};
    b64_store<0>(d, o);
    o[43] = '=';
}

}  // namespace pii
