// BGZF (blocked gzip, SAM specification section 4.1) and DEFLATE (RFC 1951) for both sides of the link: the header parser,
// the Huffman table builder with its validity checks and the per-symbol decode step are __host__ __device__ code, so the
// serial host inflater (bgzf.hip: snpgpu_bgzf_read_range, and what a sanitizer build runs over malformed files) and the
// device kernel (bgzf.hip: k_bgzf_inflate) decode with the same statements.  What differs between the two is where the
// compressed bytes come from (`In`: load32) and where the text goes (`Out`: lit, copy, sync), which the caller supplies.
//
// Malformed input is ordinary input here: every read is bounded by the length the caller gives, every write by ISIZE, every
// loop iteration consumes at least one input bit or produces at least one byte, and a bad stream ends in a status, never a trap.
#pragma once

#include <stdint.h>

#include "../../include/snpgpu.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BGZF_HD __host__ __device__ inline
#else
#define BGZF_HD inline
#endif

#define BGZF_MAX_ISIZE 65536u
#define BGZF_LIT_FAST_BITS 10u
#define BGZF_DIST_FAST_BITS 8u
#define BGZF_CL_FAST_BITS 7u

// ---- block header ---------------------------------------------------------------------------------------------------
// The block that starts at p[0] with `avail` bytes behind it; `first`: it is the first block of the file (so a mismatch means
// "this is not gzip" instead of "bad magic in mid-file").  Fills coff-relative fields of *b (csize, isize, crc, data_off).
// bgzf_parse_header reads the gzip header and its extra field only (csize, data_off); bgzf_parse_block also the footer.
BGZF_HD int bgzf_parse_header(const uint8_t *p, uint64_t avail, bool first, snpgpu_bgzf_block *b) {
    const uint8_t magic[3] = {0x1f, 0x8b, 0x08};
    if (first && (avail < 2 || p[0] != magic[0] || p[1] != magic[1])) return SNPGPU_BGZF_E_NOT_GZIP;
    for (uint32_t i = 0; i < 3 && i < avail; ++i)
        if (p[i] != magic[i]) return first ? SNPGPU_BGZF_E_NOT_BGZF : SNPGPU_BGZF_E_MAGIC;
    if (avail < 4) return SNPGPU_BGZF_E_TRUNCATED;
    if ((p[3] & 4) == 0 || (p[3] & ~4u) != 0) return SNPGPU_BGZF_E_NOT_BGZF;      // FEXTRA and nothing else (no name, comment, header CRC)
    if (avail < 12) return SNPGPU_BGZF_E_TRUNCATED;
    const uint32_t xlen = p[10] | ((uint32_t)p[11] << 8);
    if (avail < 12ull + xlen) return SNPGPU_BGZF_E_TRUNCATED;
    uint32_t bsize = 0;
    bool found = false;
    for (uint32_t o = 0; o + 4 <= xlen;) {                  // subfields: SI1 SI2 SLEN(2) data
        const uint8_t *s = p + 12 + o;
        const uint32_t slen = s[2] | ((uint32_t)s[3] << 8);
        if (o + 4 + slen > xlen) return SNPGPU_BGZF_E_NOT_BGZF;
        if (s[0] == 'B' && s[1] == 'C' && slen == 2 && !found) { bsize = s[4] | ((uint32_t)s[5] << 8); found = true; }
        o += 4 + slen;
    }
    if (!found) return SNPGPU_BGZF_E_NOT_BGZF;
    const uint32_t csize = bsize + 1;
    if (csize < 12 + xlen + 8) return SNPGPU_BGZF_E_MAGIC;  // no room for its own header and footer: not a block header
    b->csize = csize;
    b->data_off = 12 + xlen;
    return SNPGPU_OK;
}
BGZF_HD int bgzf_parse_block(const uint8_t *p, uint64_t avail, bool first, snpgpu_bgzf_block *b) {
    const int rc = bgzf_parse_header(p, avail, first, b);
    if (rc != SNPGPU_OK) return rc;
    if (avail < b->csize) return SNPGPU_BGZF_E_TRUNCATED;
    const uint8_t *f = p + b->csize - 8;
    b->crc = f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | ((uint32_t)f[3] << 24);
    b->isize = f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) | ((uint32_t)f[7] << 24);
    if (b->isize > BGZF_MAX_ISIZE) return SNPGPU_BGZF_E_ISIZE;
    return SNPGPU_OK;
}

// ---- CRC-32 (the gzip polynomial, reflected) --------------------------------------------------------------------------
#define BGZF_CRC_POLY 0xedb88320u
BGZF_HD uint32_t bgzf_crc_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ BGZF_CRC_POLY : c >> 1;
    return c;
}
// a(x) * b(x) mod p(x) in the reflected representation (bit 31 is x^0)
BGZF_HD uint32_t bgzf_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ BGZF_CRC_POLY : b >> 1;
    }
    return p;
}
// crc32(A || B) from crc32(A), crc32(B) and the length of B: crc_a * x^(8 * len_b) + crc_b over GF(2)
BGZF_HD uint32_t bgzf_crc_shift(uint32_t crc_a, uint32_t len_b) {
    uint32_t p = 1u << 31, sq = 1u << 23;                   // x^0, x^8
    for (uint32_t n = len_b; n; n >>= 1) {
        if (n & 1) p = bgzf_crc_mul(sq, p);
        sq = bgzf_crc_mul(sq, sq);
    }
    return bgzf_crc_mul(p, crc_a);
}

// ---- Huffman tables ---------------------------------------------------------------------------------------------------
// Everything a block's decoder indexes dynamically lives here (LDS on the device, the stack on the host).
struct BgzfTables {
    uint16_t lit_fast[1u << BGZF_LIT_FAST_BITS];   // (symbol << 4) | code length for codes of up to 10 bits, 0 for longer ones
    uint16_t dist_fast[1u << BGZF_DIST_FAST_BITS];
    uint16_t cl_fast[1u << BGZF_CL_FAST_BITS];
    uint16_t lit_sym[288], dist_sym[32], cl_sym[20];       // symbols in canonical order (by length, then value)
    uint16_t lit_count[16], dist_count[16], cl_count[16];  // codes per length
    uint16_t offs[16];
    uint8_t lens[288 + 32];
};
struct BgzfHuff { uint16_t *fast, *sym, *count; uint32_t fast_bits; };

// Canonical code of n symbols with lengths lens[i] <= 15.  Returns 0, or 1 when the set is over-subscribed, or incomplete
// in any way but the one zlib accepts (a single code of length 1).  A set without any code is accepted (a block without
// matches has no distance code): decoding with it finds no symbol.
BGZF_HD int bgzf_build(const BgzfHuff &h, const uint8_t *lens, uint32_t n, uint16_t *offs) {
    for (uint32_t l = 0; l < 16; ++l) h.count[l] = 0;
    for (uint32_t i = 0; i < n; ++i) h.count[lens[i] & 15] = (uint16_t)(h.count[lens[i] & 15] + 1);
    for (uint32_t i = 0; i < (1u << h.fast_bits); ++i) h.fast[i] = 0;
    if (h.count[0] == n) return 0;
    int32_t left = 1;
    uint32_t max_len = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        left = left * 2 - (int32_t)h.count[l];
        if (left < 0) return 1;
        if (h.count[l]) max_len = l;
    }
    if (left > 0 && max_len != 1) return 1;
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = lens[i] & 15;
        if (l) { h.sym[offs[l]] = (uint16_t)i; offs[l] = (uint16_t)(offs[l] + 1); }
    }
    uint32_t code = 0, idx = 0;
    for (uint32_t l = 1; l <= h.fast_bits; ++l) {
        for (uint32_t k = 0; k < h.count[l]; ++k, ++idx, ++code) {
            uint32_t rev = 0;
            for (uint32_t b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1 - b);
            const uint16_t e = (uint16_t)(((uint32_t)h.sym[idx] << 4) | l);
            for (uint32_t f = rev; f < (1u << h.fast_bits); f += 1u << l) h.fast[f] = e;
        }
        code <<= 1;
    }
    return 0;
}

// ---- bit reader -------------------------------------------------------------------------------------------------------
// In::load32(off): the four bytes at deflate-data offset `off`, little endian, zero beyond the end of the data.
template <class In>
struct BgzfBits {
    In &in;
    uint64_t buf = 0;
    uint32_t n = 0;             // valid bits in buf
    uint32_t next = 0;          // data offset of the next byte to load
    BGZF_HD explicit BgzfBits(In &i) : in(i) {}
    BGZF_HD void fill() { if (n <= 32) { buf |= (uint64_t)in.load32(next) << n; next += 4; n += 32; } }     // at least 32 bits afterwards
    BGZF_HD uint32_t peek(uint32_t k) const { return (uint32_t)buf & ((1u << k) - 1u); }    // k <= 16
    BGZF_HD void drop(uint32_t k) { buf >>= k; n -= k; }
    BGZF_HD uint32_t take(uint32_t k) { fill(); const uint32_t v = peek(k); drop(k); return v; }
    BGZF_HD uint64_t consumed_bits() const { return (uint64_t)next * 8 - n; }
};

// One symbol; -1 when the next 15 bits are no code of the set.  Consumes at least one bit.
template <class In>
BGZF_HD int32_t bgzf_decode(BgzfBits<In> &br, const BgzfHuff &h) {
    br.fill();
    const uint32_t e = h.fast[br.peek(h.fast_bits)];
    if (e & 15u) { br.drop(e & 15u); return (int32_t)(e >> 4); }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        code |= br.peek(1);
        br.drop(1);
        const uint32_t c = h.count[l];
        if (code - first < c) return (int32_t)h.sym[index + (code - first)];      // (code >= first always)
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

BGZF_HD uint32_t bgzf_cl_order(uint32_t i) {                // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    const uint64_t a = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t b = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return i < 12 ? (uint32_t)(a >> (5 * i)) & 31u : (uint32_t)(b >> (5 * (i - 12))) & 31u;
}

// ---- one BGZF block's deflate stream --------------------------------------------------------------------------------------
// in_bytes: the deflate data (between the gzip header and the CRC32/ISIZE footer); isize: what the footer promises.
// Out::lit(pos, byte), Out::copy(pos, dist, len) write the text window [0, isize) — the caller of these has checked
// pos < isize, pos + len <= isize and dist <= pos — and Out::sync() orders the table stores of one step before the loads
// of the next (a workgroup barrier on the device, nothing on the host).  Returns a SNPGPU_BGZF_ST_* status; *produced is
// the number of text bytes written.  The CRC is the caller's to check.
template <class In, class Out>
BGZF_HD uint32_t bgzf_inflate(In &in, uint32_t in_bytes, Out &out, uint32_t isize, BgzfTables *t, uint32_t *produced) {
    BgzfBits<In> br(in);
    const uint64_t total_bits = (uint64_t)in_bytes * 8;
    const BgzfHuff lit{t->lit_fast, t->lit_sym, t->lit_count, BGZF_LIT_FAST_BITS};
    const BgzfHuff dist{t->dist_fast, t->dist_sym, t->dist_count, BGZF_DIST_FAST_BITS};
    const BgzfHuff cl{t->cl_fast, t->cl_sym, t->cl_count, BGZF_CL_FAST_BITS};
    uint32_t pos = 0;
    *produced = 0;
    for (;;) {
        const uint32_t hdr = br.take(3);
        if (br.consumed_bits() > total_bits) return SNPGPU_BGZF_ST_INPUT_END;
        const uint32_t bfinal = hdr & 1u, btype = hdr >> 1;
        if (btype == 3) return SNPGPU_BGZF_ST_BTYPE;
        if (btype == 0) {
            br.drop(br.n & 7u);                                     // to the byte boundary
            const uint32_t len = br.take(16), nlen = br.take(16);
            if (br.consumed_bits() > total_bits) return SNPGPU_BGZF_ST_INPUT_END;
            if ((len ^ 0xFFFFu) != nlen) return SNPGPU_BGZF_ST_STORED_LEN;
            uint32_t at = (uint32_t)(br.consumed_bits() >> 3);      // whole bytes still in the bit buffer go back
            br.buf = 0; br.n = 0;
            if ((uint64_t)at + len > in_bytes) return SNPGPU_BGZF_ST_INPUT_END;
            if (pos + len > isize) return SNPGPU_BGZF_ST_OUTPUT_OVER;
            for (uint32_t i = 0; i < len; i += 4) {
                const uint32_t w = in.load32(at + i);
                for (uint32_t k = 0; k < 4 && i + k < len; ++k) out.lit(pos + i + k, (uint8_t)(w >> (8 * k)));
            }
            pos += len;
            br.next = at + len;
        } else {
            if (btype == 1) {
                for (uint32_t i = 0; i < 288; ++i) t->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
                for (uint32_t i = 0; i < 32; ++i) t->lens[288 + i] = 5;
                out.sync();
                (void)bgzf_build(lit, t->lens, 288, t->offs);
                out.sync();
                (void)bgzf_build(dist, t->lens + 288, 32, t->offs);
                out.sync();
            } else {
                const uint32_t hlit = br.take(5) + 257, hdist = br.take(5) + 1, hclen = br.take(4) + 4;
                if (hlit > 286 || hdist > 30) return SNPGPU_BGZF_ST_CODE_SET;
                for (uint32_t i = 0; i < 19; ++i) t->lens[i] = 0;
                out.sync();
                for (uint32_t i = 0; i < hclen; ++i) t->lens[bgzf_cl_order(i)] = (uint8_t)br.take(3);
                if (br.consumed_bits() > total_bits) return SNPGPU_BGZF_ST_INPUT_END;
                out.sync();
                if (bgzf_build(cl, t->lens, 19, t->offs)) return SNPGPU_BGZF_ST_CODE_SET;
                out.sync();
                // the literal/length lengths and the distance lengths are ONE sequence: a repeat may run from the first into the second
                const uint32_t n_lens = hlit + hdist;
                uint32_t i = 0, prev = 0;
                while (i < n_lens) {
                    const int32_t s = bgzf_decode(br, cl);
                    if (br.consumed_bits() > total_bits) return SNPGPU_BGZF_ST_INPUT_END;
                    if (s < 0) return SNPGPU_BGZF_ST_CODE_SET;
                    uint32_t rep = 1, val = (uint32_t)s;
                    if (s == 16) {
                        if (i == 0) return SNPGPU_BGZF_ST_CODE_SET;     // nothing to repeat
                        val = prev; rep = 3 + br.take(2);
                    } else if (s == 17) { val = 0; rep = 3 + br.take(3); }
                    else if (s == 18) { val = 0; rep = 11 + br.take(7); }
                    if (i + rep > n_lens) return SNPGPU_BGZF_ST_CODE_SET;
                    for (uint32_t k = 0; k < rep; ++k) t->lens[(i + k < hlit ? 0 : 288 - hlit) + i + k] = (uint8_t)val;
                    i += rep;
                    prev = val;
                }
                if (br.consumed_bits() > total_bits) return SNPGPU_BGZF_ST_INPUT_END;
                for (uint32_t k = hlit; k < 288; ++k) t->lens[k] = 0;
                for (uint32_t k = hdist; k < 32; ++k) t->lens[288 + k] = 0;
                out.sync();
                if (t->lens[256] == 0) return SNPGPU_BGZF_ST_CODE_SET;  // no end-of-block code: the block could never end
                if (bgzf_build(lit, t->lens, 288, t->offs)) return SNPGPU_BGZF_ST_CODE_SET;
                out.sync();
                if (bgzf_build(dist, t->lens + 288, 32, t->offs)) return SNPGPU_BGZF_ST_CODE_SET;
                out.sync();
            }
            for (;;) {
                const int32_t s = bgzf_decode(br, lit);
                if (br.consumed_bits() > total_bits) return SNPGPU_BGZF_ST_INPUT_END;
                if (s < 0 || s > 285) return SNPGPU_BGZF_ST_SYMBOL;
                if (s < 256) {
                    if (pos >= isize) return SNPGPU_BGZF_ST_OUTPUT_OVER;
                    out.lit(pos, (uint8_t)s);
                    ++pos;
                    continue;
                }
                if (s == 256) break;
                const uint32_t k = (uint32_t)s - 257;
                uint32_t len;
                if (k < 8) len = 3 + k;
                else if (k == 28) len = 258;
                else { const uint32_t x = (k >> 2) - 1; len = 3 + ((4 + (k & 3)) << x) + br.take(x); }
                const int32_t ds = bgzf_decode(br, dist);
                if (ds < 0 || ds > 29) return br.consumed_bits() > total_bits ? SNPGPU_BGZF_ST_INPUT_END : SNPGPU_BGZF_ST_SYMBOL;
                uint32_t d;
                if (ds < 4) d = 1 + (uint32_t)ds;
                else { const uint32_t x = ((uint32_t)ds >> 1) - 1; d = 1 + ((2 + ((uint32_t)ds & 1)) << x) + br.take(x); }
                if (br.consumed_bits() > total_bits) return SNPGPU_BGZF_ST_INPUT_END;
                if (d > pos) return SNPGPU_BGZF_ST_DISTANCE;            // before the block's own first byte
                if (pos + len > isize) return SNPGPU_BGZF_ST_OUTPUT_OVER;
                out.copy(pos, d, len);
                pos += len;
            }
        }
        *produced = pos;
        if (bfinal) break;
    }
    *produced = pos;
    return pos < isize ? SNPGPU_BGZF_ST_OUTPUT_SHORT : SNPGPU_BGZF_ST_OK;
}
