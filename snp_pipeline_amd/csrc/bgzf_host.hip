// BGZF on the host, without a context and without the HIP runtime: the probe, the block index, the serial inflater of one block
// (the decode statements of bgzf_core.h, which the kernel of bgzf.hip runs too) and the plain bytes at an offset.  This file
// and bgzf_core.h are all a stand-alone program needs to run the decoder over malformed files under a sanitizer
// (tools/probe/bgzf_host_check.hip).
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <vector>

#include "bgzf_core.h"
#include "bgzf_host.h"

namespace {

// ---- host side of the shared decoder ----------------------------------------------------------------------------------
struct HostIn {
    const uint8_t *p;
    uint32_t n;
    uint32_t load32(uint32_t off) const {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k)
            if ((uint64_t)off + k < n) v |= (uint32_t)p[off + k] << (8 * k);
        return v;
    }
};
struct HostOut {
    uint8_t *w;
    void lit(uint32_t pos, uint8_t c) { w[pos] = c; }
    void copy(uint32_t pos, uint32_t dist, uint32_t len) { for (uint32_t i = 0; i < len; ++i) w[pos + i] = w[pos + i - dist]; }
    void sync() {}
};

uint32_t host_crc32(const uint8_t *p, uint32_t n) {
    struct Table { uint32_t v[256]; };
    static const Table table_once = [] {                    // (a function-local static: initialised once, whichever thread comes first)
        Table t;
        for (uint32_t i = 0; i < 256; ++i) t.v[i] = bgzf_crc_table_entry(i);
        return t;
    }();
    const uint32_t *table = table_once.v;
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}

bool block_table_entry_ok(const snpgpu_bgzf_block &b) {
    return b.csize <= 65536u && b.data_off >= 12 && (uint64_t)b.data_off + 8 <= b.csize && b.isize <= BGZF_MAX_ISIZE;
}

}  // namespace

bool snpgpu_bgzf_block_entry_ok(const snpgpu_bgzf_block &b) { return block_table_entry_ok(b); }

int snpgpu_bgzf_index_file(const char *path, std::vector<snpgpu_bgzf_block> &blocks, snpgpu_bgzf_info *info, const uint8_t **map, uint64_t *map_bytes) {
    *map = nullptr;
    *map_bytes = 0;
    snpgpu_bgzf_info local;
    if (!info) info = &local;
    memset(info, 0, sizeof *info);
    info->bad_block = ~0ull;
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    struct stat stt;
    if (fd < 0 || fstat(fd, &stt) != 0 || !S_ISREG(stt.st_mode)) {
        if (fd >= 0) close(fd);
        return SNPGPU_E_IO;
    }
    const uint64_t n = (uint64_t)stt.st_size;
    const uint8_t *p = nullptr;
    if (n) {
        void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) { close(fd); return SNPGPU_E_IO; }
        p = (const uint8_t *)m;
    }
    close(fd);
    uint64_t count = 0;
    int rc = snpgpu_bgzf_index(p, n, nullptr, 0, &count, info);
    if (rc == SNPGPU_OK) {
        blocks.resize(count);
        rc = snpgpu_bgzf_index(p, n, blocks.data(), count, &count, info);
    }
    if (rc != SNPGPU_OK) { if (p) munmap((void *)p, n); return rc; }
    *map = p;
    *map_bytes = n;
    return SNPGPU_OK;
}

extern "C" {

const char *snpgpu_bgzf_strerror(int code) {
    switch (code) {
        case SNPGPU_OK: return "no error";
        case SNPGPU_BGZF_E_NOT_GZIP: return "not a gzip file";
        case SNPGPU_BGZF_E_NOT_BGZF: return "gzip without the BGZF block-size subfield: recompress with bgzip";
        case SNPGPU_BGZF_E_TRUNCATED: return "truncated: a BGZF block runs past the end of the data";
        case SNPGPU_BGZF_E_ISIZE: return "a BGZF block promises more than 65536 bytes of text";
        case SNPGPU_BGZF_E_MAGIC: return "bad BGZF block header in mid-file";
        case SNPGPU_E_IO: return "cannot open or read the file";
        default: return "unknown BGZF error";
    }
}

const char *snpgpu_bgzf_status_name(uint32_t st) {
    static const char *const names[] = {"ok", "reserved deflate block type", "stored block LEN/NLEN mismatch", "invalid code length set",
                                        "invalid symbol in the deflate stream", "match distance before the start of the block",
                                        "deflate stream ends before its end-of-block code", "more text than ISIZE", "less text than ISIZE", "CRC32 mismatch"};
    return st < sizeof names / sizeof names[0] ? names[st] : "unknown status";
}

int snpgpu_bgzf_probe(const char *path) {
    if (!path) return SNPGPU_E_ARG;
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return SNPGPU_E_IO;
    struct stat stt;
    if (fstat(fd, &stt) != 0 || !S_ISREG(stt.st_mode)) { close(fd); return SNPGPU_E_IO; }
    uint8_t hdr[12 + 65535];
    size_t got = 0;
    // the fixed part first, the extra field (where BC may stand behind other subfields) only when there is one
    size_t want = 12;
    for (int round = 0; round < 2; ++round) {
        while (got < want) {
            const ssize_t r = pread(fd, hdr + got, want - got, (off_t)got);
            if (r < 0) { if (errno == EINTR) continue; close(fd); return SNPGPU_E_IO; }
            if (r == 0) break;
            got += (size_t)r;
        }
        if (got < 12 || hdr[0] != 0x1f || hdr[1] != 0x8b || hdr[2] != 8 || !(hdr[3] & 4)) break;
        want = 12 + (hdr[10] | ((size_t)hdr[11] << 8));
    }
    close(fd);
    snpgpu_bgzf_block b;
    const int rc = bgzf_parse_header(hdr, got, true, &b);   // (the header alone: whether the block's data is all there is the index's business)
    if (rc == SNPGPU_BGZF_E_NOT_GZIP) return 0;
    if (rc == SNPGPU_OK) return 1;
    return rc;
}

int snpgpu_bgzf_index(const uint8_t *data, uint64_t nbytes, snpgpu_bgzf_block *out_blocks, uint64_t capacity, uint64_t *out_n, snpgpu_bgzf_info *info) {
    snpgpu_bgzf_info local;
    if (!info) info = &local;
    memset(info, 0, sizeof *info);
    info->bad_block = ~0ull;
    info->compressed_bytes = nbytes;
    if (out_n) *out_n = 0;
    if (nbytes && !data) return SNPGPU_E_ARG;
    uint64_t off = 0, poff = 0, n = 0;
    bool last_is_eof = false;
    int rc = SNPGPU_OK;
    while (off < nbytes) {
        snpgpu_bgzf_block b{};
        rc = bgzf_parse_block(data + off, nbytes - off, n == 0, &b);
        if (rc != SNPGPU_OK) { info->bad_block = n; info->bad_offset = off; break; }
        b.coff = off;
        b.poff = poff;
        if (n < capacity && out_blocks) out_blocks[n] = b;
        last_is_eof = b.isize == 0 && b.csize == 28;
        off += b.csize;
        poff += b.isize;
        ++n;
    }
    info->n_blocks = n;
    info->plain_bytes = poff;
    info->index_rc = rc;
    info->has_eof_marker = rc == SNPGPU_OK && last_is_eof ? 1u : 0u;
    if (out_n) *out_n = n;
    return rc;
}

uint32_t snpgpu_bgzf_inflate_block_host(const uint8_t *block, const snpgpu_bgzf_block *b, uint8_t *out) {
    if (!block || !b || !block_table_entry_ok(*b) || (b->isize && !out)) return SNPGPU_BGZF_ST_INPUT_END;
    BgzfTables tables;
    HostIn in{block + b->data_off, b->csize - b->data_off - 8};
    HostOut wout{out};
    uint32_t produced = 0;
    uint32_t st = bgzf_inflate(in, in.n, wout, b->isize, &tables, &produced);
    if (st == SNPGPU_BGZF_ST_OK && host_crc32(out, b->isize) != b->crc) st = SNPGPU_BGZF_ST_CRC;
    return st;
}

int snpgpu_bgzf_read_range(const char *path, uint64_t plain_offset, uint64_t nbytes, uint8_t *out, uint64_t *out_n) {
    if (out_n) *out_n = 0;
    if (!path || (nbytes && !out)) return SNPGPU_E_ARG;
    std::vector<snpgpu_bgzf_block> blocks;
    const uint8_t *map = nullptr;
    uint64_t map_bytes = 0;
    int rc = snpgpu_bgzf_index_file(path, blocks, nullptr, &map, &map_bytes);
    if (rc != SNPGPU_OK) return rc;
    // the first block whose text ends behind the offset
    size_t lo = 0, hi = blocks.size();
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (blocks[mid].poff + blocks[mid].isize <= plain_offset) lo = mid + 1; else hi = mid;
    }
    std::vector<uint8_t> text(BGZF_MAX_ISIZE);
    uint64_t done = 0;
    for (size_t i = lo; i < blocks.size() && done < nbytes; ++i) {
        const snpgpu_bgzf_block &b = blocks[i];
        if (!b.isize) continue;
        if (snpgpu_bgzf_inflate_block_host(map + b.coff, &b, text.data()) != SNPGPU_BGZF_ST_OK) { rc = SNPGPU_E_PILEUP; break; }
        const uint64_t from = plain_offset + done - b.poff;
        uint64_t take = b.isize - from;
        if (take > nbytes - done) take = nbytes - done;
        memcpy(out + done, text.data() + from, take);
        done += take;
    }
    if (map) munmap((void *)map, map_bytes);
    if (out_n) *out_n = done;
    return rc;
}

}  // extern "C"
