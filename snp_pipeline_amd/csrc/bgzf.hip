// BGZF-compressed pileups: the inflate kernel on the device (the block index and the serial host inflater: bgzf_host.hip).
//
// A pileup is text that compresses several-fold, and everything this library does with a file is bound by the host link
// (stream.hip), so the bytes that cross it should be the compressed ones.  BGZF cuts the text into gzip members of at most
// 64 KiB, each with its compressed size in the header: the host finds the blocks by hopping from header to header
// (snpgpu_bgzf_index), the kernel inflates them independently.
//
// k_bgzf_inflate: one wave (a workgroup of 64 lanes) per block.  DEFLATE is a serial bit stream, so the wave decodes it in
// lock step — every lane holds the same bit buffer and walks the same tables (LDS reads of one address broadcast) — and
// uses its 64 lanes where the work is wide: refilling the input window, copying a match, the CRC32 of the text (a slice
// per lane, combined over GF(2)) and the store of the text to global memory.  The block's whole text window (64 KiB), the
// input window (1 KiB) and the Huffman tables live in LDS: two blocks per CU.  History never passes through global memory,
// so there is no question of one lane reading back stale bytes another lane stored.  The decode statements themselves are
// those of bgzf_core.h, shared with the host inflater.
#include <string.h>

#include <vector>

#include "bgzf_core.h"
#include "internal.h"

namespace {

// ---- device side ------------------------------------------------------------------------------------------------------------
#define BGZF_RING_BYTES 1024u
struct BgzfLds {
    uint8_t win[BGZF_MAX_ISIZE];                // the block's text
    uint32_t ring[BGZF_RING_BYTES / 4];         // deflate data [wend - 1024, wend), filled 512 bytes at a time
    uint32_t crc_table[256];
    BgzfTables tables;
};

struct DevIn {
    const uint8_t *g;           // the deflate data in global memory (any alignment)
    uint32_t n;                 // its length: no byte at or behind g + n is read
    uint32_t *ring;
    uint32_t wend;              // the ring holds the data up to here (a multiple of 512)
    uint32_t lane;
    __device__ void advance() {
        const uint32_t o = wend + lane * 8;
        uint32_t lo = 0, hi = 0;
        if (o + 8 <= n && (((uintptr_t)(g + o)) & 7) == 0) {
            const uint2 v = *(const uint2 *)(g + o);
            lo = v.x; hi = v.y;
        } else {
            for (uint32_t k = 0; k < 4; ++k) if (o + k < n) lo |= (uint32_t)g[o + k] << (8 * k);
            for (uint32_t k = 0; k < 4; ++k) if (o + 4 + k < n) hi |= (uint32_t)g[o + 4 + k] << (8 * k);
        }
        __syncthreads();                                    // every lane has read what it wanted from the half that is overwritten
        ring[(o >> 2) & (BGZF_RING_BYTES / 4 - 1)] = lo;
        ring[((o >> 2) + 1) & (BGZF_RING_BYTES / 4 - 1)] = hi;
        wend += 512;
        __syncthreads();
    }
    __device__ uint32_t load32(uint32_t off) {
        if (off >= n) return 0;                             // (also what bounds the loop below: wend passes n after at most n / 512 + 1 rounds)
        while (off + 4 > wend) advance();
        const uint32_t lo = ring[(off >> 2) & (BGZF_RING_BYTES / 4 - 1)], hi = ring[((off >> 2) + 1) & (BGZF_RING_BYTES / 4 - 1)];
        const uint32_t sh = (off & 3) * 8;
        return sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    }
};

struct DevOut {
    uint8_t *w;
    uint32_t lane;
    __device__ void lit(uint32_t pos, uint8_t c) { if (lane == 0) w[pos] = c; }
    // pos + len <= isize and dist <= pos have been checked; the source bytes all lie before pos, also when dist < len
    __device__ void copy(uint32_t pos, uint32_t dist, uint32_t len) {
        __syncthreads();
        const uint8_t *src = w + pos - dist;
        for (uint32_t i = lane; i < len; i += 64) w[pos + i] = src[dist >= len ? i : dist == 1 ? 0 : i % dist];
        __syncthreads();
    }
    __device__ void sync() { __syncthreads(); }
};

__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint8_t *__restrict__ comp, const snpgpu_bgzf_block *__restrict__ blocks, uint32_t n_blocks,
                                                     uint8_t *out, uint32_t *status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t bgzf_lds_raw[];
    BgzfLds &L = *(BgzfLds *)bgzf_lds_raw;
    const uint32_t lane = threadIdx.x;
    const uint32_t blk = blockIdx.x;
    if (blk >= n_blocks) return;
    const snpgpu_bgzf_block b = blocks[blk];
    for (uint32_t i = lane; i < 256; i += 64) L.crc_table[i] = bgzf_crc_table_entry(i);
    const uint32_t isize = b.isize <= BGZF_MAX_ISIZE ? b.isize : BGZF_MAX_ISIZE;      // (the host has checked the table; the window is the bound here)
    const uint32_t in_bytes = b.csize - b.data_off - 8;
    DevIn in{comp + b.coff + b.data_off, in_bytes, L.ring, 0, lane};
    DevOut wout{L.win, lane};
    __syncthreads();
    uint32_t produced = 0;
    uint32_t st = bgzf_inflate(in, in_bytes, wout, isize, &L.tables, &produced);
    __syncthreads();
    if (st == SNPGPU_BGZF_ST_OK) {
        // CRC32: a slice per lane (an odd number of dwords, so that the lanes' reads spread over the banks), then
        // crc(A || B) = crc(A) * x^(8 |B|) + crc(B): every lane shifts its own by the bytes behind its slice
        uint32_t per = ((isize + 63) / 64 + 3) & ~3u;
        if (((per >> 2) & 1) == 0) per += 4;
        const uint32_t lo = lane * per < isize ? lane * per : isize, hi = lo + per < isize ? lo + per : isize;
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t i = lo; i < hi; ++i) c = L.crc_table[(c ^ L.win[i]) & 0xFF] ^ (c >> 8);
        c = hi > lo ? ~c : 0;
        uint32_t x = hi > lo ? bgzf_crc_shift(c, isize - hi) : 0;
        for (int off = 32; off; off >>= 1) x ^= __shfl_xor(x, off);
        if (x != b.crc) st = SNPGPU_BGZF_ST_CRC;
    }
    if (st == SNPGPU_BGZF_ST_OK && isize) {
        // the text: bytes up to the first 16-byte boundary of the destination, 16 bytes per lane from there, bytes at the end
        uint8_t *dst = out + b.poff;
        uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
        if (head > isize) head = isize;
        const uint32_t n_vec = (isize - head) / 16, tail0 = head + n_vec * 16;
        if (lane < head) dst[lane] = L.win[lane];
        const uint32_t *w32 = (const uint32_t *)L.win;
        const uint32_t sh = (head & 3) * 8;
        for (uint32_t v = lane; v < n_vec; v += 64) {
            const uint32_t s = (head + v * 16) >> 2;        // the dword of the window that holds the first byte
            uint32_t a[5];
            for (uint32_t k = 0; k < 4; ++k) a[k] = w32[s + k];
            a[4] = sh ? w32[s + 4 < BGZF_MAX_ISIZE / 4 ? s + 4 : s + 3] : 0;       // (sh != 0: the 16 bytes end inside dword s + 4, which is inside the window)
            uint4 o;
            o.x = sh ? (a[0] >> sh) | (a[1] << (32 - sh)) : a[0];
            o.y = sh ? (a[1] >> sh) | (a[2] << (32 - sh)) : a[1];
            o.z = sh ? (a[2] >> sh) | (a[3] << (32 - sh)) : a[2];
            o.w = sh ? (a[3] >> sh) | (a[4] << (32 - sh)) : a[3];
            *(uint4 *)(dst + head + v * 16) = o;
        }
        for (uint32_t i = tail0 + lane; i < isize; i += 64) dst[i] = L.win[i];
    }
    if (lane == 0) status[blk] = st;
}

}  // namespace

// ---- internal interface (internal.h) ------------------------------------------------------------------------------------
size_t snpgpu_bgzf_scratch_bytes(uint64_t n_blocks) { return (size_t)n_blocks * (sizeof(snpgpu_bgzf_block) + 4) + 512; }

int snpgpu_bgzf_check_table(snpgpu_ctx *ctx, const snpgpu_bgzf_block *h_blocks, uint64_t n_blocks, uint64_t compressed_bytes, uint64_t out_capacity) {
    if (n_blocks > 0x7FFFFFFFull) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "too many BGZF blocks in one call");
    for (uint64_t i = 0; i < n_blocks; ++i) {
        const snpgpu_bgzf_block &b = h_blocks[i];
        if (!snpgpu_bgzf_block_entry_ok(b) || b.coff > compressed_bytes || b.csize > compressed_bytes - b.coff)
            return snpgpu_set_error(ctx, SNPGPU_E_ARG, "BGZF block %llu of the table leaves the compressed data", (unsigned long long)i);
        if (b.poff > out_capacity || b.isize > out_capacity - b.poff)
            return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the text of BGZF block %llu would pass the output buffer (%llu + %u > %llu)", (unsigned long long)i,
                                    (unsigned long long)b.poff, b.isize, (unsigned long long)out_capacity);
    }
    return SNPGPU_OK;
}

// d_ws: snpgpu_bgzf_scratch_bytes(n_blocks); the status words are at *d_status afterwards (n_blocks of them).  The table has been checked.
int snpgpu_enqueue_bgzf_inflate(snpgpu_ctx *ctx, const uint8_t *d_comp, const snpgpu_bgzf_block *h_blocks, uint64_t n_blocks, uint8_t *d_out, void *d_ws,
                                uint32_t **d_status) {
    snpgpu_bgzf_block *d_blocks = (snpgpu_bgzf_block *)d_ws;
    *d_status = (uint32_t *)((char *)d_ws + ((n_blocks * sizeof(snpgpu_bgzf_block) + 255) & ~(size_t)255));
    if (!n_blocks) return SNPGPU_OK;
    if (!ctx->bgzf_lds_attr) {
        (void)hipFuncSetAttribute((const void *)k_bgzf_inflate, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        ctx->bgzf_lds_attr = true;
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_blocks, h_blocks, n_blocks * sizeof(snpgpu_bgzf_block), hipMemcpyHostToDevice, ctx->stream));
    hipEvent_t ta = snpgpu_time_begin(ctx);
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((uint32_t)n_blocks), dim3(64), sizeof(BgzfLds), ctx->stream, d_comp, d_blocks, (uint32_t)n_blocks, d_out, *d_status);
    snpgpu_time_end(ctx, SNPGPU_K_BGZF, ta);
    HIP_TRY(ctx, hipGetLastError());
    return SNPGPU_OK;
}

void snpgpu_bgzf_summarise(const snpgpu_bgzf_block *h_blocks, const uint32_t *h_status, uint64_t n_blocks, snpgpu_bgzf_info *info) {
    if (!info) return;
    info->n_bad = 0;
    for (uint64_t i = 0; i < n_blocks; ++i) {
        if (h_status[i] == SNPGPU_BGZF_ST_OK) continue;
        if (!info->n_bad) { info->bad_block = i; info->bad_offset = h_blocks[i].coff; info->bad_status = h_status[i]; }
        ++info->n_bad;
    }
}

extern "C" {

int snpgpu_bgzf_inflate_dev(snpgpu_ctx *ctx, const void *d_compressed, uint64_t compressed_bytes, const snpgpu_bgzf_block *h_blocks, uint64_t n_blocks,
                            void *d_out, uint64_t out_capacity, uint32_t *h_block_status, snpgpu_bgzf_info *info) {
    if (!ctx || (n_blocks && (!h_blocks || !d_compressed))) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (info) { memset(info, 0, sizeof *info); info->bad_block = ~0ull; info->n_blocks = n_blocks; info->compressed_bytes = compressed_bytes; }
    int rc = snpgpu_bgzf_check_table(ctx, h_blocks, n_blocks, compressed_bytes, out_capacity);
    if (rc) return rc;
    uint64_t plain = 0;
    for (uint64_t i = 0; i < n_blocks; ++i) plain += h_blocks[i].isize;
    if (info) info->plain_bytes = plain;
    if (plain && !d_out) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null output");
    if (!n_blocks) return SNPGPU_OK;
    HIP_TRY(ctx, snpgpu_enter(ctx));
    void *ws = nullptr;
    rc = snpgpu_scratch(ctx, snpgpu_bgzf_scratch_bytes(n_blocks), &ws);
    if (rc) return rc;
    uint32_t *d_status = nullptr;
    rc = snpgpu_enqueue_bgzf_inflate(ctx, (const uint8_t *)d_compressed, h_blocks, n_blocks, (uint8_t *)d_out, ws, &d_status);
    if (rc) return rc;
    std::vector<uint32_t> st(n_blocks);
    HIP_TRY(ctx, hipMemcpyAsync(st.data(), d_status, 4 * n_blocks, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (h_block_status) memcpy(h_block_status, st.data(), 4 * n_blocks);
    snpgpu_bgzf_summarise(h_blocks, st.data(), n_blocks, info);
    return SNPGPU_OK;
}

}  // extern "C"
