/* snpgpu.h — C ABI of the MI355X (gfx950) hot path of the CFSAN SNP Pipeline.
 *
 * The reference (CFSAN-Biostatistics/snp-pipeline v2.2.1) is pure Python and has
 * no FFI; its operator boundary is the `cfsan_snp_pipeline <subcommand>` CLI
 * (snppipeline/cfsan_snp_pipeline.py:309-457).  The Python host layer in
 * snp_pipeline_amd/ mirrors that CLI and calls the entry points below through
 * ctypes.  Each entry point names the reference code it replaces.
 *
 * Conventions
 *  - every function returns 0 on success, a negative SNPGPU_E_* code on failure;
 *    a message is available from snpgpu_last_error(ctx).  Nothing throws.
 *  - `*_dev` functions take DEVICE pointers, enqueue work on the context's
 *    stream and return without synchronising; the others take HOST pointers and
 *    are synchronous.  The caller owns every buffer it passes.
 *  - a context is bound to one (process, device) and is not thread-safe.
 *  - there is no CPU fallback: without a gfx950 device snpgpu_ctx_create fails.
 */
#ifndef SNPGPU_H
#define SNPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNPGPU_ABI_VERSION 7

/* ---- error codes ------------------------------------------------------- */
#define SNPGPU_OK            0
#define SNPGPU_E_HIP        -1   /* HIP runtime error (message has the hipError string) */
#define SNPGPU_E_ARG        -2   /* invalid argument */
#define SNPGPU_E_NOMEM      -3
#define SNPGPU_E_PILEUP     -4   /* malformed pileup text; see snpgpu_scan_status */
#define SNPGPU_E_UNSUPPORTED -5  /* input the reference accepts but this build refuses (reported loudly) */
#define SNPGPU_E_IO         -6   /* a file could not be opened, read or written */
#define SNPGPU_E_TIMEOUT    -7   /* snpgpu_stream_wait: the stream was still busy when the time was up */

/* ---- failed-filter bits, in the order pileup.py:564-584 appends them and
 *      call_consensus.py:165-168 appends "Region" ------------------------- */
#define SNPGPU_F_RAWDPTH  0x01
#define SNPGPU_F_VARFREQ  0x02
#define SNPGPU_F_DEPTH    0x04
#define SNPGPU_F_STRDPTH  0x08
#define SNPGPU_F_STRBIAS  0x10
#define SNPGPU_F_REGION   0x20

/* ---- site flags --------------------------------------------------------- */
#define SNPGPU_SITE_IN_SNPLIST 0x01   /* position is in snplist.txt (call_consensus.py:146) */
#define SNPGPU_SITE_EXCLUDED   0x02   /* position is in the -e exclude VCF (call_consensus.py:121) */

/* ---- per-site status ---------------------------------------------------- */
#define SNPGPU_ST_NO_LINE      0   /* no pileup line for this position: '-' (call_consensus.py:187) */
#define SNPGPU_ST_OK           1
#define SNPGPU_ST_SHORT_LINE   2   /* < 4 fields: IndexError in pileup.py:224-225 */
#define SNPGPU_ST_BAD_DEPTH    3   /* depth field is not [0-9]+: ValueError in pileup.py:225 */
#define SNPGPU_ST_NO_QUALS     4   /* depth > 0 and exactly 5 fields: IndexError in pileup.py:237 */
#define SNPGPU_ST_MULTI_REF    5   /* (ABI <= 4: reference-base field longer than SNPGPU_SPILL_REF bytes; no longer produced) */

typedef struct snpgpu_ctx snpgpu_ctx;
typedef struct snpgpu_siteset snpgpu_siteset;
typedef struct snpgpu_pileups snpgpu_pileups;

/* ConsensusCaller parameters, pileup.py:433-465 (+ Reader's min_base_quality, pileup.py:384). */
typedef struct snpgpu_caller_params {
    int32_t min_base_quality;       /* -q, default 0   */
    int32_t min_cons_depth;         /* -D, default 1   */
    int32_t min_cons_strand_depth;  /* -d, default 0   */
    int32_t reserved;
    double  min_cons_freq;          /* -c, default 0.6 */
    double  min_cons_strand_bias;   /* -b, default 0.0 */
} snpgpu_caller_params;

/* Everything pileup.Record exposes for one position (pileup.py:58-94), with the
 * histograms as a ranked list (count descending, byte ascending, pileup.py:263-266).
 * 128 bytes per site.  Enough to write consensus.vcf rows (vcf_writer.py:295-379). */
#define SNPGPU_MAX_SYMS 8
typedef struct snpgpu_site_counts {
    uint32_t raw_depth;             /* Record.raw_depth */
    uint32_t good_depth;            /* Record.good_depth */
    uint32_t fwd_good_depth;        /* Record.forward_good_depth */
    uint32_t rev_good_depth;        /* Record.reverse_good_depth */
    uint32_t n_symbols;             /* bits 0-7: distinct upper-cased symbols with good depth; when that is more than 8, or the
                                     * reference-base field has more than one byte: bits 8-31 = 1 + index of the position's
                                     * snpgpu_symbol_spill record (0xFFFFFF: there was no room) */
    uint8_t  ref_base;              /* Record.reference_base (its first byte), case preserved */
    uint8_t  cons_base;             /* ConsensusCaller.call_consensus()[0] */
    uint8_t  filters;               /* SNPGPU_F_* mask, incl. REGION */
    uint8_t  status;                /* SNPGPU_ST_* */
    uint8_t  sym[SNPGPU_MAX_SYMS];  /* most_common_good_bases[0..8) */
    uint32_t total[SNPGPU_MAX_SYMS];/* base_good_depth[sym] */
    uint32_t fwd[SNPGPU_MAX_SYMS];  /* forward_base_good_depth[sym] */
    uint32_t rev[SNPGPU_MAX_SYMS];  /* reverse_base_good_depth[sym] */
} snpgpu_site_counts;

/* Ranks 8, 9, ... of a position with more than SNPGPU_MAX_SYMS distinct symbols (pileup.py:259-266 ranks any number of them and
 * vcf_writer.py:317-331 lists every one as an ALT allele): the record itself keeps the first eight, the rest goes to one of
 * the records the context holds (SNPGPU_SPILL_CAP to begin with; more after a call that ran out: snpgpu_symbol_spill_read).  The same record carries a reference-base field of more than one byte
 * (pileup.py:223 takes any string; every '.' / ',' then stands for all of its characters, pileup.py:255-258, and the VCF
 * REF column shows the string): ref_len > 1 and ref[] hold it, n may be 0.  And a depth column outside 0 .. 2^32 - 1 (depth64).  A call that produces per-site records starts with an empty spill;
 * snpgpu_symbol_spill_read copies out what the context's calls have put there since (synchronises the context's stream). */
#define SNPGPU_SPILL_SYMS 120
#define SNPGPU_SPILL_REF  64
#define SNPGPU_SPILL_CAP  1024
typedef struct snpgpu_symbol_spill {
    uint32_t n;                         /* entries used */
    uint32_t ref_len;                   /* 0 or 1: the record's ref_base is the whole field; else the field's length: its first
                                         * SNPGPU_SPILL_REF bytes in ref[], the rest — raw, no header — in the
                                         * ceil((ref_len - SNPGPU_SPILL_REF) / sizeof(record)) records that follow this one (ref[] is
                                         * the last member, so the field is one run of bytes starting at ref) */
    int64_t  depth64;                   /* Record.raw_depth when the record's 32 unsigned bits cannot hold it — int() takes "-3"
                                         * and "5000000000" (pileup.py:225) and consensus.vcf prints what it got; else 0 */
    uint8_t  sym[SNPGPU_SPILL_SYMS];    /* most_common_good_bases[8 + k] */
    uint32_t total[SNPGPU_SPILL_SYMS];
    uint32_t fwd[SNPGPU_SPILL_SYMS];
    uint32_t rev[SNPGPU_SPILL_SYMS];
    uint8_t  ref[SNPGPU_SPILL_REF];     /* Record.reference_base when it is longer than one byte, case preserved */
} snpgpu_symbol_spill;

/* Result words of one pileup scan (device-written, 4 x u64). */
#define SNPGPU_SCAN_STATUS_WORDS 4
/*  [0] first malformed line: ((byte offset + 1) << 8) | code, or UINT64_MAX when clean
 *        code 1: line has < 2 fields      (ValueError at pileup.py:425)
 *        code 2: position is not [0-9]+   (ValueError at pileup.py:426)
 *        code 3: byte >= 0x80 in the file (non-ASCII pileup: unsupported)
 *  [1] number of lines seen, [2] number of lines that matched a site, [3] sum of the depth column over
 *      well-formed lines (collect_metrics.py:325-340 by-product; 0 unless requested) */

/* ---- context ------------------------------------------------------------ */
int  snpgpu_abi_version(void);
int  snpgpu_device_count(void);   /* visible gfx950 devices (0 when there is no usable HIP runtime); creates no context */
int  snpgpu_ctx_create(int device, snpgpu_ctx **out);
void snpgpu_ctx_destroy(snpgpu_ctx *ctx);
const char *snpgpu_last_error(const snpgpu_ctx *ctx);
/* Run on the caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL is HIP's default stream.
 * snpgpu_ctx_reset_stream goes back to the context's own non-blocking stream. */
int  snpgpu_ctx_set_stream(snpgpu_ctx *ctx, void *hip_stream);
int  snpgpu_ctx_reset_stream(snpgpu_ctx *ctx);
int  snpgpu_ctx_sync(snpgpu_ctx *ctx);

/* ---- the CPU budget of the host side (ABI 7) ------------------------------------------------------------------------------
 * Replaces run.py:387-400 (MaxCpuCores: min(psutil.cpu_count(), MaxCpuCores) caps the reference's per-sample process fan-out).
 * Here one process per GPU does its shard's host work on threads (file readers, text writers), so the cap is divided among the
 * processes that share the node:
 *   usable_cpus = min(CPUs in the affinity mask, the cgroup's CPU quota (v2 cpu.max / v1 cfs quota), max_cpu_cores)
 *   budget      = max(1, usable_cpus / local_ranks)        -> readers, writers (what the entry points start by default)
 * max_cpu_cores: snpgpu_set_max_cpu_cores, else the environment variable SNPGPU_MAX_CPU_CORES, else no cap.
 * local_ranks:   snpgpu_set_local_ranks, else SNPGPU_LOCAL_RANKS, else LOCAL_WORLD_SIZE (torch.distributed.run), else 1.
 * An explicit thread count in a call's options (snpgpu_stream_opts.n_readers, n_threads arguments) still wins. */
typedef struct snpgpu_cpu_budget_info {
    uint32_t affinity_cpus;              /* sched_getaffinity */
    uint32_t quota_cpus;                 /* cgroup quota / period, rounded down, at least 1; 0 = no quota */
    uint32_t max_cpu_cores;              /* the cap in force; 0 = none */
    uint32_t usable_cpus;
    uint32_t local_ranks;
    uint32_t budget;                     /* CPUs this process plans with */
    uint32_t readers;                    /* default reader threads of the file entry points */
    uint32_t writers;                    /* default formatting threads of the text writers / the FASTA survey */
} snpgpu_cpu_budget_info;
int  snpgpu_cpu_budget(snpgpu_cpu_budget_info *out);
void snpgpu_set_max_cpu_cores(uint32_t cores);   /* 0 = back to the environment / no cap */
void snpgpu_set_local_ranks(uint32_t ranks);     /* 0 = back to the environment / 1 */
/* Kernel-only elapsed time helpers (HIP events recorded on the context's stream). */
int  snpgpu_timer_start(snpgpu_ctx *ctx);
int  snpgpu_timer_stop_ms(snpgpu_ctx *ctx, float *out_ms);   /* synchronises on the stop event */

/* Per-kernel timing for bench.py: when enabled, HIP events are recorded on the stream around every launch of
 * the scan (0), per-site caller (1) and distance (2) kernels, around everything phase-1 site calling launches for a
 * file (3) and around the VCF count of a piece of a file (4); snpgpu_ctx_kernel_time_ms synchronises, returns the
 * summed elapsed time and the number of launches of that kernel since the last query, and clears them. */
int  snpgpu_ctx_kernel_timing(snpgpu_ctx *ctx, int enable);
int  snpgpu_ctx_kernel_time_ms(snpgpu_ctx *ctx, int kernel, float *total_ms, uint32_t *launches);

/* ---- site set: the (chrom,pos) set handed to pileup.Reader (pileup.py:396-403) ----
 * contig_names: concatenated names, contig_name_off[n_contigs+1]; names must be sorted bytewise and unique.
 * site_keys: (contig_index << 32) | position, strictly increasing; site_flags: SNPGPU_SITE_* per key.
 * All HOST pointers; the set is copied to the device (bitmap + rank directory). */
int  snpgpu_siteset_create(snpgpu_ctx *ctx, const uint8_t *contig_names, const uint32_t *contig_name_off,
                           uint32_t n_contigs, const uint64_t *site_keys, const uint8_t *site_flags,
                           uint32_t n_sites, snpgpu_siteset **out);
void snpgpu_siteset_destroy(snpgpu_siteset *ss);
uint32_t snpgpu_siteset_size(const snpgpu_siteset *ss);

/* ---- call_consensus: pileup.Reader + Record + ConsensusCaller + the mapping in
 *      call_consensus.py:161-188, for ONE sample ------------------------------------------------
 * d_pileup: raw ASCII of reads.all.pileup in device memory (any alignment).
 * d_out_base[n_sites]:    the byte call_consensus.py writes to the FASTA for that key ('-' when a filter failed,
 *                         the base is '*', or the position has no line).
 * d_out_filters[n_sites]: SNPGPU_F_* mask (0 when the position has no line).
 * d_out_counts[n_sites]:  nullable.
 * d_status[4]:            SNPGPU_SCAN_STATUS_WORDS u64.
 * want_depth_sum: also accumulate status[3] (costs one integer parse per line). */
int  snpgpu_call_consensus_dev(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const void *d_pileup, size_t nbytes,
                               const snpgpu_caller_params *params, uint8_t *d_out_base, uint8_t *d_out_filters,
                               snpgpu_site_counts *d_out_counts, uint64_t *d_status, int want_depth_sum);
/* Many samples resident in one device buffer: ONE scan launch and ONE call launch serve up to 256 samples (the
 * waves of the scan are dealt to the samples in proportion to their sizes), which is what the throughput figures
 * are quoted on.  Sample i is bytes [h_offsets[i], h_offsets[i] + h_sizes[i]) of d_pileups; h_sizes == NULL means
 * the samples are packed back to back, h_sizes[i] = h_offsets[i+1] - h_offsets[i] (h_offsets then has n_samples + 1
 * entries).  Outputs are [n_samples][n_sites] row-major; d_status is [n_samples][4]. */
int  snpgpu_call_consensus_batch_dev(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const void *d_pileups,
                                     const uint64_t *h_offsets, const uint64_t *h_sizes, uint32_t n_samples,
                                     const snpgpu_caller_params *params, uint8_t *d_out_base,
                                     uint8_t *d_out_filters, uint64_t *d_status);
/* Samples anywhere in device memory (d_pileups: HOST array of n device pointers, h_sizes their lengths), with everything the
 * streamed form returns: d_out_counts (nullable) and d_out_line_off (nullable) are [n][n_sites] like the other outputs,
 * d_site_flags (nullable) [n][n_sites] replaces the set's flags per sample (a sample's own exclude list).  Asynchronous. */
int  snpgpu_call_consensus_many_dev(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const void *const *d_pileups,
                                    const uint64_t *h_sizes, uint32_t n_samples, const snpgpu_caller_params *params,
                                    const uint8_t *d_site_flags, uint8_t *d_out_base, uint8_t *d_out_filters,
                                    snpgpu_site_counts *d_out_counts, uint64_t *d_out_line_off, uint64_t *d_status,
                                    int want_depth_sum);
/* Host-buffer form for one pileup (an mmap, bytes read elsewhere): streamed through the same pipeline as
 * snpgpu_call_consensus_files below, synchronous.
 * Returns SNPGPU_E_PILEUP when the scan found a malformed line (status words still filled). */
int  snpgpu_call_consensus(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const uint8_t *pileup, size_t nbytes,
                           const snpgpu_caller_params *params, uint8_t *out_base, uint8_t *out_filters,
                           snpgpu_site_counts *out_counts, uint64_t *out_status, int want_depth_sum);
/* ---- streamed ingestion: pileup FILES -> consensus bytes --------------------------------------------------
 * Replaces the reference's input side of call_consensus: the text-mode line iterator over the open pileup
 * (pileup.py:408-429, driven from call_consensus.py:161) and the one-process-per-sample job array around it
 * (run.py:704-718).  Reader threads pread() the files in chunks of whole 4 KiB scan tiles into pinned staging
 * buffers, a copy stream moves each chunk into the file's device buffer, and the scan runs over the tiles that
 * have landed while the rest of the file is still on its way; the exact parser's queue and the call step run
 * when the file is complete.  Files alternate between device buffers, so the next file streams in during the
 * tail of the previous one.  No file is ever resident in host memory as a whole.
 *
 * Outputs are [n_files][n_sites] row-major HOST arrays: out_base / out_filters as snpgpu_call_consensus_dev,
 * out_counts (nullable) the per-site records, out_line_off (nullable) 1 + byte offset of the line used for
 * each site (0 = none), out_status [n_files][4] the scan status words, out_rc (nullable) per file: 0,
 * SNPGPU_E_IO (could not open / read: its outputs are void), SNPGPU_E_PILEUP or SNPGPU_E_UNSUPPORTED (malformed
 * pileup: see its status words).  The return value is 0 unless the pipeline itself failed.
 *
 * excl_off / excl_slots (both nullable): per-file exclude lists (call_consensus.py:117-123: every sample of step 7.2 has its
 * own var.flt_removed.vcf) as CSR over site-set slots — file f is called with the set's flags plus SNPGPU_SITE_EXCLUDED on
 * slots excl_slots[excl_off[f] .. excl_off[f+1]), so one site set (the union of the snplist and every file's list) and one
 * stream of files serve all samples. */
typedef struct snpgpu_stream_opts {      /* 0 = default everywhere */
    uint32_t chunk_bytes;                /* bytes per host->device copy (default 8 MiB; rounded up to 4 KiB) */
    uint32_t n_staging;                  /* pinned staging buffers (default: readers + 4) */
    uint32_t n_readers;                  /* reader threads (default: snpgpu_cpu_budget().readers — 8 on a big host, fewer on a small one or beside other ranks) */
    uint32_t n_slots;                    /* device file buffers = files in flight (default 2) */
    uint32_t want_depth_sum;             /* also accumulate status[3] (collect_metrics.py:325-340 by-product) */
    uint32_t reserved[3];
} snpgpu_stream_opts;
typedef struct snpgpu_stream_stats {
    uint64_t bytes;                      /* pileup bytes that went through */
    uint64_t n_chunks;
    double   seconds;                    /* wall time of the call */
    double   seconds_waiting_for_readers;/* ... of which the issuing thread waited for a chunk to be read */
    double   seconds_waiting_for_device; /* ... and for the device to finish a file */
    uint32_t n_readers, n_staging, chunk_bytes, reserved;
    double   reader_seconds_reading;     /* summed over the reader threads: inside pread / memcpy */
    double   reader_seconds_waiting;     /* ... waiting for a staging buffer to be copied out */
    double   seconds_enqueueing;         /* issuing thread: inside HIP enqueue calls (copies, events, kernels) */
} snpgpu_stream_stats;
int  snpgpu_call_consensus_files(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const char *const *paths, uint32_t n_files,
                                 const snpgpu_caller_params *params, const uint32_t *excl_off, const uint32_t *excl_slots,
                                 uint8_t *out_base, uint8_t *out_filters,
                                 snpgpu_site_counts *out_counts, uint64_t *out_line_off, uint64_t *out_status,
                                 int32_t *out_rc, const snpgpu_stream_opts *opts, snpgpu_stream_stats *stats);
/* The same stream with its rows left ON THE DEVICE: d_out_base / d_out_filters / d_out_counts (nullable) / d_out_line_off (nullable)
 * are [n_files][n_sites] row-major DEVICE arrays, the layout snpgpu_call_consensus_many_dev writes — the kernels of file f write
 * row f, so a group of pileups that was never resident is ready for snpgpu_region_flow_dev / snpgpu_group_check_dev when the
 * call returns (synchronous, like the host form).  out_status [n_files][4] and out_rc [n_files] (nullable) stay HOST arrays: the
 * caller decides per file without reading device memory.  The rows of a file with out_rc == SNPGPU_E_IO are written as '-' / 0 /
 * no line / zeroed records.  The spill records of all files of the call form one arena (snpgpu_symbol_spill_read serves every
 * row).  Every other argument as snpgpu_call_consensus_files.  (Additive in ABI 7.) */
int  snpgpu_call_consensus_files_dev(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const char *const *paths, uint32_t n_files,
                                     const snpgpu_caller_params *params, const uint32_t *excl_off, const uint32_t *excl_slots,
                                     uint8_t *d_out_base, uint8_t *d_out_filters,
                                     snpgpu_site_counts *d_out_counts, uint64_t *d_out_line_off, uint64_t *out_status,
                                     int32_t *out_rc, const snpgpu_stream_opts *opts, snpgpu_stream_stats *stats);

/* call_consensus --vcfAllPos (call_consensus.py:148-151, pileup.py:418-421): a Record for EVERY line of the pileup,
 * whether its position is listed or not.  Synchronous; host outputs in file order: out_line_off[i] = 1 + byte offset of
 * line i, out_line_flags[i] = SNPGPU_SITE_* of its position (0 when it is not in the site set), out_counts[i] its
 * record (filters include REGION for excluded positions).  *out_n_lines is always set; when it exceeds `capacity`
 * nothing else is written and the caller comes back with larger arrays (capacity 0 just counts the lines).
 * out_status[4]: [0] first line whose chrom / position columns are malformed (else UINT64_MAX), [1] lines. */
int  snpgpu_call_all_lines_file(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const char *path,
                                const snpgpu_caller_params *params, uint64_t capacity, uint64_t *out_n_lines,
                                uint64_t *out_line_off, uint8_t *out_line_flags, snpgpu_site_counts *out_counts,
                                uint64_t *out_status);

/* The same pass with 32-byte records (ABI 7).  Nearly every line of a pileup has at most three distinct symbols and depths far
 * below 65 536: such a line's record is packed into a snpgpu_line_record — everything consensus.vcf prints for it
 * (vcf_writer.py:295-379) — and only the others ("wide": more symbols, a count above 65 535, a spill record, a Record-level error)
 * come back as the full 128-byte record, with their line index.  5 M lines: 200 MB over the host link instead of 685 MB.
 *   good_depth = total[0] + total[1] + total[2], forward_good_depth = sum of fwd[], reverse_good_depth = sum of rev[]
 * (each kept read base counts for exactly one symbol; a line is only packed when these sums hold).
 * out_records[i] is line i of the file (n_symbols == SNPGPU_LINE_WIDE: look the line up in out_wide_index, ascending, and take
 * out_wide[k]).  *out_n_wide is always set; when it exceeds wide_capacity (or *out_n_lines exceeds capacity) nothing else is
 * written and the caller comes back with larger arrays.  Other arguments and the status words as snpgpu_call_all_lines_file. */
#define SNPGPU_LINE_WIDE 0xFF
#define SNPGPU_LINE_SYMS 3
typedef struct snpgpu_line_record {
    uint32_t raw_depth;                     /* Record.raw_depth */
    uint16_t total[SNPGPU_LINE_SYMS];       /* base_good_depth of the ranked symbols */
    uint16_t fwd[SNPGPU_LINE_SYMS];
    uint16_t rev[SNPGPU_LINE_SYMS];
    uint8_t  sym[SNPGPU_LINE_SYMS];         /* most_common_good_bases[0..3) */
    uint8_t  ref_base, cons_base, filters, status;      /* as in snpgpu_site_counts */
    uint8_t  n_symbols;                     /* 0 .. 3, or SNPGPU_LINE_WIDE */
    uint8_t  site_flags;                    /* SNPGPU_SITE_* of the line's position (0: not in the site set) */
    uint8_t  reserved;
} snpgpu_line_record;
int  snpgpu_call_all_lines_compact_file(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const char *path,
                                        const snpgpu_caller_params *params, uint64_t capacity, uint64_t *out_n_lines,
                                        uint64_t *out_line_off, snpgpu_line_record *out_records,
                                        uint32_t wide_capacity, uint32_t *out_n_wide, uint32_t *out_wide_index,
                                        snpgpu_site_counts *out_wide, uint64_t *out_status);

/* Rows of consensus.vcf from such records, host code (no device): the lines [0, n_lines) of the pileup text `pileup[0, nbytes)`, CHROM and
 * POS of a row from the line's own first two fields (POS as int() prints it), the numbers from records[i] — or, where that says
 * SNPGPU_LINE_WIDE, from the entry of wide[] whose wide_index equals i (ascending) — laid out as vcf_writer.py:295-379 does.
 * only_listed: rows for lines with site_flags != 0 only.  Returns the bytes the rows take and writes at most `capacity` of them to out
 * (capacity 0: just the size); *out_n_rows rows; *out_bad_line: -1, or the line whose record the writer refuses (more symbols than it
 * keeps and no spill record; an offset outside the text) — nothing is returned then. */
size_t snpgpu_format_line_rows(const uint8_t *pileup, uint64_t nbytes, const uint64_t *line_off, const snpgpu_line_record *records,
                               uint64_t n_lines, const uint32_t *wide_index, const snpgpu_site_counts *wide, uint32_t n_wide,
                               const char *const *filter_names, int preserve_ref_case, char failed_snp_gt,
                               const snpgpu_symbol_spill *spill, uint32_t n_spill, int only_listed, char *out, size_t capacity,
                               uint64_t *out_n_rows, int64_t *out_bad_line);

/* call_consensus --vcfAllPos from file to file: every row of consensus.vcf (call_consensus.py:148-151, vcf_writer.py:381-435: one
 * row per pileup LINE, in file order; CHROM and POS are the line's own first two fields, POS as int() prints it) formatted by the
 * library's host threads from the 32-byte records, straight into vcf_path behind `header` (the text of the header lines).
 * only_listed != 0: rows for the lines whose position is in the site set only (a pileup that repeats positions: the reference
 * writes a row for every matching line, call_consensus.py:178-180).  The file is written only when no line stops the reference:
 *   returns SNPGPU_E_PILEUP / SNPGPU_E_UNSUPPORTED with out_status as snpgpu_call_all_lines_file for a malformed chrom / position
 *   column; returns SNPGPU_OK with *out_first_bad_line != UINT64_MAX (and that line's record and offset + 1) when `check` is set
 *   and a Record cannot be built from some line (status > SNPGPU_ST_OK) — the caller raises what the reference raises.
 * *out_n_rows: rows written.  filter_names, preserve_ref_case, failed_snp_gt as snpgpu_format_vcf_rows. */
int  snpgpu_write_all_positions_vcf(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const char *pileup_path,
                                    const snpgpu_caller_params *params, const char *vcf_path, const char *header,
                                    const char *const *filter_names, int preserve_ref_case, char failed_snp_gt,
                                    int only_listed, int check, uint64_t *out_n_lines, uint64_t *out_n_rows,
                                    uint64_t *out_first_bad_line, uint64_t *out_first_bad_off, snpgpu_site_counts *out_first_bad,
                                    uint64_t *out_status);

/* ---- phase-1 site calling: the counting + selection half of `VarScan mpileup2snp` -------------------------------
 * Replaces what call_sites.py:89-108 gets from the VarScan v2.3.9 jar (a third-party dependency that is not in the
 * reference tree): VarScan.qualityDepth, VarScan.getReadCounts and the min-coverage / min-reads2 / min-avg-qual /
 * min-var-freq tests of VarScan.callPosition, for every line of a one-sample pileup.  Each (line, allele) that passes
 * leaves one record; Fisher's exact test, --p-value, the strand filter and the VCF text are host work on those
 * records (snp_pipeline_amd/varscan.py). */
typedef struct snpgpu_varscan_params {
    uint32_t min_coverage;          /* --min-coverage, default 8: raw depth AND qualities >= min_avg_qual */
    uint32_t min_reads2;            /* --min-reads2, default 2 (the pipeline passes 5) */
    uint32_t min_avg_qual;          /* --min-avg-qual, default 15 */
    uint32_t reserved;
    double   min_var_freq;          /* --min-var-freq, default 0.20 (the pipeline passes 0.90) */
} snpgpu_varscan_params;
typedef struct snpgpu_varscan_site {
    uint64_t line_off;              /* byte offset of the pileup line in the file (chrom / position text are read there) */
    uint32_t sdp;                   /* depth column */
    uint32_t dp;                    /* qualities >= min_avg_qual */
    uint32_t total;                 /* reads over all alleles at that quality + indel-carrying reads: FREQ's denominator */
    uint32_t rdf, rdr, ref_qual_sum;/* '.' / ',' at that quality, and the sum of their qualities */
    uint32_t adf, adr, alt_qual_sum;/* the same for alt_base */
    uint8_t  ref_base, alt_base;    /* upper case */
    uint8_t  reserved[2];
} snpgpu_varscan_site;
/* path -> records in file order (ties: allele A < C < G < T).  Streams the file to the device, indexes its lines, runs
 * the kernel, copies the records back; synchronous.  *out_n_sites is the number of records found; when it exceeds
 * `capacity` only `capacity` arbitrary ones were written and the caller comes back with a larger array.
 * out_status[2]: [0] byte offset of the first malformed line (fewer than six non-empty TAB-separated columns, a depth
 * that is not a plain integer, a reference column longer than one byte) else UINT64_MAX — the call then returns
 * SNPGPU_E_PILEUP; [1] lines in the file.  SNPGPU_E_IO when the file cannot be read. */
int  snpgpu_varscan_file(snpgpu_ctx *ctx, const char *path, const snpgpu_varscan_params *params, uint32_t capacity,
                         snpgpu_varscan_site *out_sites, uint32_t *out_n_sites, uint64_t *out_status);

/* Many files in one call: the reader threads run ahead across file boundaries, the files alternate between two device
 * slots, and a file's kernels run while the next file is read and copied (the shape of snpgpu_call_consensus_files).
 * out_sites is [n_files][capacity], out_n_sites [n_files], out_status [n_files][2], out_rc [n_files] (SNPGPU_OK, SNPGPU_E_IO or
 * SNPGPU_E_PILEUP per file; the call itself fails only for argument, memory or HIP errors).  A file with more records
 * than `capacity` reports its count in out_n_sites and leaves out_sites undefined for it: repeat it with
 * snpgpu_varscan_file. */
int  snpgpu_varscan_files(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, const snpgpu_varscan_params *params,
                          uint32_t capacity, snpgpu_varscan_site *out_sites, uint32_t *out_n_sites, uint64_t *out_status,
                          int32_t *out_rc);

/* The same over a pileup that already is in device memory. */
int  snpgpu_varscan_dev(snpgpu_ctx *ctx, const void *d_pileup, uint64_t nbytes, const snpgpu_varscan_params *params,
                        uint32_t capacity, snpgpu_varscan_site *out_sites, uint32_t *out_n_sites, uint64_t *out_status);

/* The same over MANY pileups that are in device memory (the resident files of a snpgpu_pileups store, synthetic ones): one
 * scan launch over all of them — every wave works inside one file, the waves are dealt to the files by size — so the ramp and
 * the tail of a launch are paid once per call, not once per 0.1 ms file.  Arguments as snpgpu_varscan_files: out_sites is
 * [n_files][capacity], out_n_sites [n_files], out_status [n_files][2], out_rc [n_files] (SNPGPU_OK or SNPGPU_E_PILEUP per
 * file); a file with more records than `capacity` reports its count and leaves its out_sites undefined (repeat it with
 * snpgpu_varscan_dev).  At most 65 535 files per call.  What the reference does per sample with one JVM each
 * (call_sites.py:89-108, run.py:662 runs them as a job array). */
int  snpgpu_varscan_batch_dev(snpgpu_ctx *ctx, const void *const *d_pileups, const uint64_t *nbytes, uint32_t n_files,
                              const snpgpu_varscan_params *params, uint32_t capacity, snpgpu_varscan_site *out_sites,
                              uint32_t *out_n_sites, uint64_t *out_status, int32_t *out_rc);

/* ---- the SNP count of a VCF file: what collect_metrics.py:61-106 (count_vcf_file_snps, through PyVCF) returns ------------
 * The file is streamed through the staging chunks of the pileup streams and counted on the device by a text kernel.  Per data
 * line (not empty, not starting with '#'; a CR in front of the terminator is not part of it):
 *   - ten TAB-separated columns; FORMAT and the sample column split on ':' into the same number of fields, one named GT; every
 *     allele of GT (split on '/' or '|') is '.' or a decimal index into [REF] + ALT.split(','); the line is shorter than
 *     SNPGPU_VCF_LINE_WINDOW bytes.  A data line outside this grammar is UNUSUAL: it is counted as such and not judged;
 *   - not a SNP when an allele is '.', when every allele is 0, when none of the named alleles is one of the single letters
 *     A C G T N, or when there is an FT field whose value is not exactly PASS; one SNP otherwise.
 * out_counts[3]: SNPs among the usual lines, data lines, unusual lines.  out_unusual_off[capacity]: the byte offsets of the
 * first bytes of the unusual lines in ascending order (all of them when out_counts[2] <= capacity, else `capacity` arbitrary
 * ones); for a line of SNPGPU_VCF_LINE_WINDOW bytes or more the offset of its TERMINATOR with bit 63 set.  Such a line is
 * reported before its first byte is seen: a '#' line or an empty line that long is counted in out_counts[1] and [2] as well, and
 * it is the caller who reads the line (backwards from the terminator) and finds that it counts nothing.  *out_status: the
 * SNPGPU_VCF_* bits below.  Returns SNPGPU_E_IO when the file cannot be opened or read (an error of the input), another code
 * for everything else.  Synchronous. */
#define SNPGPU_VCF_LINE_WINDOW 4096
#define SNPGPU_VCF_MORE_UNUSUAL 1u  /* more unusual lines than `capacity` */
#define SNPGPU_VCF_LONG_LINE    2u  /* one of the reported lines is longer than the window */
int  snpgpu_vcf_count_snps_file(snpgpu_ctx *ctx, const char *path, uint32_t capacity, uint64_t *out_counts,
                                uint64_t *out_unusual_off, uint64_t *out_status);
/* Many files as ONE stream (the readers run ahead across file boundaries): out_counts [n_files][3], out_unusual_off
 * [n_files][capacity], out_status [n_files], out_rc [n_files] (SNPGPU_OK or SNPGPU_E_IO per file; the call itself fails only
 * for argument, memory or HIP errors). */
int  snpgpu_vcf_count_snps_files(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, uint32_t capacity,
                                 uint64_t *out_counts, uint64_t *out_unusual_off, uint64_t *out_status, int32_t *out_rc);

/* ---- merge_vcfs: the multi-sample VCF file from the per-sample files of this pipeline's own writer (vcf_merge.hip) ----------
 * paths[n_files]: the files in COLUMN order, each with one sample column; out_path: the merged file (created or truncated);
 * own_lines[own_len]: header lines of the caller (each with its LF) that go in front of #CHROM, where bcftools puts its two.
 * The files are streamed through the staging ring; a kernel turns every data line inside the grammar (see vcf_merge.hip) into
 * a record, the site union is a sort + unique, one wave merges a site (ALT union in column order, GT and the Number=A vectors
 * re-indexed, NS summed, FILTER united), and the text is formatted on the device and written by the library's writer threads.
 * A line outside the kernel's grammar, or longer than SNPGPU_VCF_LINE_WINDOW, is parsed on the host, one line at a time
 * (stats->host_lines counts them); a line outside the host's rule as well, a position that comes twice in one file, or records of
 * different REF at one position end the call with SNPGPU_E_UNSUPPORTED and a message that names the file and the byte offset
 * (also in stats->bad_file / bad_offset); nothing is dropped silently.  SNPGPU_E_IO: a file cannot be read or written.
 * The text leaves the device in rounds of sites: as many whole rows as the output buffer holds are formatted, copied back in
 * 16 MiB pieces and written, then the next (stats->rounds); the buffer is 64 MiB, or 2^options bytes for options 12 to 32, and
 * never shorter than the longest row.  snpgpu_merge_vcf_files is the single pass: the records and the [site][column] table
 * are held whole, 160 bytes a record and 4 bytes a sample cell, at most 2^31 - 2 records.  Synchronous. */
typedef struct snpgpu_merge_stats {
    uint64_t columns, sites, cells, host_lines, bytes;          /* bytes: the size of the merged file */
    uint64_t bad_file, bad_offset;                              /* of the line that ended the call (UINT64_MAX: none) */
    double   seconds_parse, seconds_merge, seconds_write;       /* reading + parsing; union, rows and formatting; copy back + pwrite */
    uint32_t writer_threads, rounds;                            /* rounds: ranges of sites the text went out in */
} snpgpu_merge_stats;
int  snpgpu_merge_vcf_files(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, const char *out_path,
                            const char *own_lines, uint32_t own_len, uint32_t options, snpgpu_merge_stats *stats);

/* The merge at any size, in bounded device memory.  snpgpu_merge_plan (host only: no device, no context) says how a merge of
 * n_files files with n_sites sites and total_input_bytes bytes of input runs under a budget of device bytes:
 *   - the single pass above (input_passes 1, site_rounds 0) when its footprint fits: the record bound (one record per 56 bytes
 *     of input plus room for 65 600), the key, sort and table arrays by the dense bound (every column a record at every site), the
 *     row arrays, the output buffer and the stream's three piece buffers — figures of the input's size alone, so the route is
 *     chosen before a byte is read;
 *   - else a key pass and site_rounds passes, 1 + site_rounds readings of the input.  The key pass streams the files through a
 *     kernel that keeps 24 bytes of a line (CHROM hash, POS, column, offset), in batches of as many keys as an eighth of the budget
 *     past the stream's buffers holds (at least 4096), each sorted, uniqued and folded into the running site union: O(batch +
 *     sites) bytes.  Then, for every
 *     range of sites_per_round sites of the union, the files are streamed again, a record whose (contig, POS) ranks inside the
 *     range goes to its slot [site - lo][column] (164 bytes a slot), and rows and text follow as in the single pass, appended to
 *     the file.  sites_per_round is the most whole sites whose slots, row arrays and output buffer (planned at 256 + 48 bytes a
 *     column per row, never more than 2^out_buffer_log2; a longer row gets its length) fit beside the union and the key
 *     pass's arrays (freed by then, and counted all the same: every number of sites a round has a budget), and at most
 *     (2^31 - 2) / n_files, and n_sites - 1 where the single pass could run but does not fit (the round of all sites is the
 *     single pass).  passes->device_bytes: the bytes the plan holds.
 * device_bytes 0: for snpgpu_merge_plan no budget at all, for the merge the device's free memory at the call less the larger of
 * 1 GiB and a sixteenth of it.  SNPGPU_E_NOMEM: the budget is below the key pass and one site's round (passes->device_bytes: the
 * bytes needed); the merge names them in its message and writes nothing.
 * snpgpu_merge_vcf_files_opts follows that plan (passes, when given, reports it).  Results, errors, messages and stats are those of
 * the single pass on the same input; stats->host_lines counts a host-parsed line once, cells and sites are totals, rounds sums
 * the ranges of sites the text went out in.  The bounded form writes to a sibling of out_path and renames it at the end: after an
 * error out_path is as it was before the call.  (Where two errors sit in different site rounds the one of the earlier round is
 * reported.) */
typedef struct snpgpu_merge_opts {
    uint32_t out_buffer_log2;   /* 0, or 12..32: as `options` of snpgpu_merge_vcf_files */
    uint32_t reserved;
    uint64_t device_bytes;      /* budget for everything the merge allocates on the device; 0: see above */
    uint64_t reserved2[2];
} snpgpu_merge_opts;
typedef struct snpgpu_merge_passes {
    uint32_t input_passes;      /* 1 = the single pass; else 1 + site_rounds */
    uint32_t site_rounds;
    uint64_t sites_per_round;
    uint64_t device_bytes;      /* what the plan holds (after SNPGPU_E_NOMEM: what it would need) */
} snpgpu_merge_passes;
int  snpgpu_merge_plan(uint32_t n_files, uint64_t n_sites, uint64_t total_input_bytes, const snpgpu_merge_opts *opts,
                       snpgpu_merge_passes *out);
int  snpgpu_merge_vcf_files_opts(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, const char *out_path,
                                 const char *own_lines, uint32_t own_len, const snpgpu_merge_opts *opts,
                                 snpgpu_merge_stats *stats, snpgpu_merge_passes *passes /* may be NULL */);

/* ---- resident pileups: the input side of the one-job pipeline (`cfsan_snp_pipeline hot_path_batch`) ----------------------
 * The reference runs steps 4-11 as separate process arrays over a shared file system (run.py:662-784): call_sites
 * (call_sites.py:89-108) and call_consensus twice (run.py:704-710, :712-718) each read a sample's reads.all.pileup again.
 * A snpgpu_pileups store keeps the files in device memory instead: snpgpu_pileups_ingest streams them in exactly as
 * snpgpu_varscan_files does (same reader threads, staging ring, copy streams; site calling on a file while the next one
 * arrives) but leaves every file where it landed, while `budget_bytes` of device memory last (0: what is free at creation
 * less 24 GiB); files past the budget are site-called through the two streaming slots and stay non-resident.  The consensus
 * step then reads the resident files with snpgpu_call_consensus_many_dev: each pileup crosses the host link once.
 * params == NULL: no site calling (the files are only made resident).  out_done (nullable) [n_files]: set to 1 (release
 * store) when the outputs of file f are final, so that another host thread can turn them into var.flt.vcf while the call is
 * still running.  Other arguments as snpgpu_varscan_files. */
typedef struct snpgpu_pileups_stats {
    uint64_t h2d_bytes;             /* bytes copied host -> device on behalf of the store */
    uint64_t file_bytes;            /* sizes of the ingested files */
    uint64_t resident_bytes;        /* device bytes taken (files + padding) */
    uint64_t budget_bytes;
    uint32_t n_files, n_resident;
    double   seconds;                       /* wall time of the ingest calls, of which the issuing thread spent ... */
    double   seconds_allocating;            /* ... allocating device memory, */
    double   seconds_waiting_for_readers;   /* waiting for a piece of a file to be read, */
    double   seconds_waiting_for_device;    /* and waiting for the device (line counts, results) */
    double   reader_seconds_reading;        /* summed over the reader threads: inside pread */
    double   reader_seconds_waiting;        /* ... waiting for a staging buffer to be copied out */
    double   seconds_preparing;             /* part of `seconds` before the first read starts: files opened and placed, staging memory */
    uint32_t n_readers;                     /* reader threads of the last ingest call (ABI 7: from snpgpu_cpu_budget) */
    uint32_t reserved;
} snpgpu_pileups_stats;
int  snpgpu_pileups_create(snpgpu_ctx *ctx, uint64_t budget_bytes, snpgpu_pileups **out);
void snpgpu_pileups_destroy(snpgpu_pileups *store);
int  snpgpu_pileups_ingest(snpgpu_ctx *ctx, snpgpu_pileups *store, const char *const *paths, uint32_t n_files,
                           const snpgpu_varscan_params *params, uint32_t capacity, snpgpu_varscan_site *out_sites,
                           uint32_t *out_n_sites, uint64_t *out_status, int32_t *out_rc, int32_t *out_done);
uint32_t snpgpu_pileups_count(const snpgpu_pileups *store);
/* file `index` in ingestion order: its device pointer (NULL when it is not resident) and size */
int  snpgpu_pileups_get(const snpgpu_pileups *store, uint32_t index, void **d_ptr, uint64_t *nbytes);
int  snpgpu_pileups_get_stats(const snpgpu_pileups *store, snpgpu_pileups_stats *out);

/* The host half of the same step (no device work, no context): the records of snpgpu_varscan_file, in its order, ->
 * var.flt.vcf data lines.  Per line: the allele with the most variant reads among those whose Fisher p (reads against a
 * 0.1 % error model, VarScan.getSignificance) is <= p_value; strand filter (FILTER str10); GT 1/1 at or above
 * min_freq_for_hom, else 0/1; chrom and position text are taken from `pileup` (the file's bytes, e.g. an mmap) at the
 * record's line offset.  Writes at most `capacity` bytes to `out` (may be NULL), returns the bytes the lines take and
 * leaves their number in *out_rows. */
typedef struct snpgpu_varscan_finish {
    double  p_value;                /* --p-value, default 0.99 */
    double  min_freq_for_hom;       /* --min-freq-for-hom, default 0.75 */
    int32_t strand_filter;          /* --strand-filter, default 1 */
    int32_t reserved;
} snpgpu_varscan_finish;
size_t snpgpu_varscan_format_rows(const snpgpu_varscan_site *sites, uint32_t n_sites, const uint8_t *pileup,
                                  uint64_t pileup_bytes, const snpgpu_varscan_finish *fin, char *out, size_t capacity,
                                  uint32_t *out_rows);

/* consensus.vcf data lines from per-site records — host-side text formatting, no device work, no context
 * (vcf_writer.py:295-435: _make_vcf_record_from_pileup + the text PyVCF3's Writer emits for it).  Row r is the record
 * counts[order[r]] (order == NULL: r) of site site_keys[order[r]] = (contig index << 32) | position, contig names as
 * in snpgpu_siteset_create; filter_names: the six names in SNPGPU_F_* bit order; failed_snp_gt: '.', '0' or '1'.
 * spill / n_spill (nullable / 0): the context's spill records for positions with more than SNPGPU_MAX_SYMS symbols.
 * Writes at most `capacity` bytes to `out` (may be NULL) and returns the number of bytes the rows take; a record with
 * more than SNPGPU_MAX_SYMS symbols whose spill record is not in `spill` is skipped and its row index left in *out_bad_row
 * (else -1). */
size_t snpgpu_format_vcf_rows(const snpgpu_site_counts *counts, const uint32_t *order, uint32_t n_rows,
                              const uint8_t *contig_names, const uint32_t *contig_name_off, const uint64_t *site_keys,
                              const char *const *filter_names, int preserve_ref_case, char failed_snp_gt,
                              const snpgpu_symbol_spill *spill, uint32_t n_spill,
                              char *out, size_t capacity, int32_t *out_bad_row);
/* *out_n = the records the context's calls have asked for since the last call that started an empty spill; up to `capacity` of
 * them are copied to `out`.  *out_n > snpgpu_symbol_spill_capacity(ctx): the arena ran out (the records past it say "no room",
 * nothing is copied) — repeat the call: the context allocates an arena of the size this one asked for at its next call. */
int  snpgpu_symbol_spill_read(snpgpu_ctx *ctx, snpgpu_symbol_spill *out, uint32_t capacity, uint32_t *out_n);
uint32_t snpgpu_symbol_spill_capacity(const snpgpu_ctx *ctx);

/* The output files of call_consensus (call_consensus.py:178-192: consensus.fasta through Bio.SeqIO, consensus.vcf through
 * vcf_writer.SingleSampleWriter) for many (sample, flow) pairs at once, on host threads — host code, no device work, no
 * context.  Per job: fasta_path (nullable) gets ">fasta_id" and `sequence` in lines of 60; vcf_path (nullable) gets vcf_header
 * followed by one row per site whose record has status SNPGPU_ST_OK, in the order of line_off (pileup order) — with
 * site_in_flow (nullable, [n_sites]) only the sites it marks and those whose row mask carries SNPGPU_F_REGION (the parse set
 * of call_consensus.py:147-151 is the snplist plus the sample's exclude list); row_filters (nullable, [n_sites]) replaces the
 * records' own failed-filter masks.  Out: rc (0, SNPGPU_E_IO, or SNPGPU_E_UNSUPPORTED for a record with more than
 * SNPGPU_MAX_SYMS symbols that has no record in spill[n_spill]) and n_rows.  Contig names / site_keys / filter_names as snpgpu_format_vcf_rows; n_threads 0 = as
 * many as there are jobs, up to 64. */
typedef struct snpgpu_consensus_job {
    const char *fasta_path;
    const char *fasta_id;
    const uint8_t *sequence;
    uint64_t n_bases;
    const char *vcf_path;
    const char *vcf_header;
    const snpgpu_site_counts *counts;
    const uint64_t *line_off;
    const uint8_t *row_filters;
    const uint8_t *site_in_flow;
    int32_t rc;
    uint32_t n_rows;
} snpgpu_consensus_job;
int  snpgpu_write_consensus_files(snpgpu_consensus_job *jobs, uint32_t n_jobs, uint32_t n_sites, const uint8_t *contig_names,
                                  const uint32_t *contig_name_off, const uint64_t *site_keys, const char *const *filter_names,
                                  int preserve_ref_case, char failed_snp_gt, const snpgpu_symbol_spill *spill, uint32_t n_spill,
                                  uint32_t n_threads);

/* Both consensus flows from one call (run.py:704-718 calls every sample twice: at the positions of snplist.txt, and at those
 * of snplist_preserved.txt with the sample's var.flt_removed.vcf as exclude file).  From the result of the call over the FULL
 * list — d_base / d_filters / d_line_off, [n_samples][n_sites] — derives the preserved flow: d_out_base [n_samples][n_cols] =
 * the columns d_cols[n_cols] (slots of the preserved list, in its order), d_out_filters [n_samples][n_sites] = the filters,
 * and for every slot of a sample's exclude list (CSR d_excl_off[n_samples + 1] / d_excl_slots) whose position has a pileup
 * line: SNPGPU_F_REGION in the filters and '-' as its base when it is a column (d_col_of[n_sites]: column of a slot or -1) —
 * call_consensus.py:165-176.  d_err: one zeroed word, bit 0 = an exclude slot >= n_sites.  Asynchronous. */
int  snpgpu_region_flow_dev(snpgpu_ctx *ctx, const uint8_t *d_base, const uint8_t *d_filters, const uint64_t *d_line_off,
                            uint32_t n_samples, uint32_t n_sites, const uint32_t *d_cols, const int32_t *d_col_of, uint32_t n_cols,
                            const uint32_t *d_excl_off, const uint32_t *d_excl_slots, uint8_t *d_out_base, uint8_t *d_out_filters,
                            uint32_t *d_err);

/* Whole rows from one device matrix to another by index lists (ABI 7): dst row dst_index[r] <- src row src_index[r], r < n_rows; a null
 * list stands for r itself; strides and row_bytes in bytes; destination rows distinct; asynchronous on the context's stream.  The
 * one-job pipeline's gathers between its steps — the rows of a group's resident samples to their places (run.py:704-718 runs the
 * samples in any order), the packed rows into sorted-id order for the distance step (distance.py:76-84) — without leaving the
 * library's kernels. */
int  snpgpu_rows_copy_dev(snpgpu_ctx *ctx, const void *d_src, uint64_t src_stride, const uint32_t *d_src_index,
                          void *d_dst, uint64_t dst_stride, const uint32_t *d_dst_index, uint32_t n_rows, uint64_t row_bytes);

/* After a call_consensus on `ss`: for every site, 1 + the byte offset of the pileup line that was used (0 = no
 * line).  consensus.vcf rows are written in pileup order (call_consensus.py:161-180), which this recovers.
 * out_line_off[n_sites] is a HOST pointer; synchronous. */
int  snpgpu_siteset_line_offsets(snpgpu_ctx *ctx, const snpgpu_siteset *ss, uint64_t *out_line_off);

/* Which call kernel took how many sites of the most recent call launch on the context (the all-lines entry points: lines).
 * The call step runs one lane per site over windows of 128, 256 and 512 bytes, each pass over what the one before handed on (a
 * line whose terminator does not lie inside the window, counted from the 16-byte boundary at or below its first byte; a bases
 * field over 64 / 128 / 255 bytes; a malformed line; a symbol besides *ACGTN), and one wave per site for the rest — every line
 * of a sample sequenced deeper than about 240x.  out[0..2]: the three lane passes in that order; out[3]: the wave-per-site
 * kernel.  Only sites that have a line count: the sum is the number of pileup lines the scan matched to a listed site (a position
 * that several lines of one file carry counts once per line in the first pass's figure).  For a batch whose lines average more
 * than 100 bytes the 128-byte pass does not run and out[0] is 0.  A public call over more samples than one launch takes (256, or
 * 1 GiB of line-offset rows) makes several launches: the figures are those of the last.  The kernels keep the counts in device
 * memory; they are read back here, so this call waits for the stream and a call launch never does.  Before any launch: all zero. */
#define SNPGPU_CALL_PASSES 4
int  snpgpu_call_pass_counts(snpgpu_ctx *ctx, uint64_t out[SNPGPU_CALL_PASSES]);

/* ---- snp_matrix / distance: utils.calculate_sequence_distance (utils.py:1135-1165) over all pairs
 *      (distance.py:93-98) ----------------------------------------------------------------------
 * The samples x sites matrix is packed 4 bits per site, planar per 32-site word:
 *   packed[row][word] = uint32[4] { valid (upper(c) in ACGT), code bit1, code bit0, lower-case flag }
 * with A=0 C=1 G=2 T=3.  A row holds ceil(n_sites / 32) words rounded up to a multiple of 4 (64 bytes); the padding
 * words are all zero (no valid site).  snpgpu_packed_row_bytes() is the row pitch. */
size_t snpgpu_packed_row_bytes(uint32_t n_sites);
int  snpgpu_pack_matrix_dev(snpgpu_ctx *ctx, const uint8_t *d_symbols, uint32_t n_rows, uint32_t n_sites,
                            size_t row_stride, void *d_packed);
/* d_out is a full n x n int32 matrix.  Only the 128x128 tiles t of the upper triangle with
 * t % tile_nranks == tile_rank are computed; each is written together with its mirror image.
 * Entries of other tiles are left untouched. */
int  snpgpu_distance_packed_dev(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites,
                                uint32_t tile_rank, uint32_t tile_nranks, int32_t *d_out);
/* Host form: symbols is n_rows x n_sites bytes (row-major, the sequences of snpma.fasta); out is n x n int32. */
int  snpgpu_distance(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, int32_t *out);

/* The first two columns of every record of a VCF (host code): what utils.convert_vcf_file_to_snp_set (utils.py:1113-1132)
 * and filter_regions.py:408-410 read through PyVCF3.  out_pos / out_contig [capacity] in file order (contig = index into
 * the file's names in order of first appearance, returned back to back in out_names with out_name_off[n_names + 1]);
 * *out_n_records may exceed `capacity` (then only the count is valid: come back with more room), SNPGPU_E_NOMEM: more
 * room for the names.  Plain files only — TAB-separated, POS of plain digits below 2^32, header before data: anything else
 * is SNPGPU_E_UNSUPPORTED and belongs to the caller's own reader. */
int  snpgpu_vcf_sites(const char *path, uint64_t capacity, uint32_t *out_pos, uint32_t *out_contig, uint64_t *out_n_records,
                      char *out_names, uint64_t names_capacity, uint64_t *out_name_off, uint32_t names_max,
                      uint32_t *out_n_names);
/* The first two columns of snplist.txt, what utils.read_snp_position_list (utils.py:1073-1088) returns: as snpgpu_vcf_sites,
 * but every line is a record (no header, no blank lines); a line outside the plain case — columns separated by anything but
 * TAB, a position that is not 1-10 plain digits — is SNPGPU_E_UNSUPPORTED and belongs to the caller's own reader. */
int  snpgpu_snplist_sites(const char *path, uint64_t capacity, uint32_t *out_pos, uint32_t *out_contig, uint64_t *out_n_records,
                          char *out_names, uint64_t names_capacity, uint64_t *out_name_off, uint32_t names_max,
                          uint32_t *out_n_names);
/* snplist.txt (utils.write_list_of_snps, utils.py:1056-1070): one "chrom\tpos\tcount\tname..." line per site; keys =
 * (contig index << 32) | pos in output order, carriers of site i = carriers[carrier_off[i], carrier_off[i+1]) as sample
 * indices; contig / sample names back to back with their offset arrays. */
int  snpgpu_write_snplist(const char *path, const char *contig_names, const uint64_t *contig_off, const uint64_t *keys,
                          uint64_t n_sites, const uint32_t *carrier_off, const uint32_t *carriers, const char *sample_names,
                          const uint64_t *sample_off);

/* snpma.fasta into a byte matrix (host code, no device work): replaces the read loop of distance.py:76-84 — text-mode lines
 * ("\n", "\r\n", lone "\r"), a line that starts with '>' opens a record named by the rest of the line without its leading
 * '>'s, every other line is appended to the current record.  Two passes: snpgpu_fasta_scan counts the records, the longest
 * sequence and the bytes of all names (SNPGPU_E_UNSUPPORTED: sequence text before the first header, which the reference
 * cannot handle either); snpgpu_fasta_load fills out_matrix (record r at r * row_stride, padded with `pad` up to row_stride
 * >= the longest sequence), out_len[n_records], and the names back to back with out_name_off[n_records + 1].  Records keep
 * the file's order and its duplicates (the reference's dict keeps the last of equal names: the caller's business). */
int  snpgpu_fasta_scan(const char *path, uint64_t *out_n_records, uint64_t *out_max_len, uint64_t *out_names_bytes);
int  snpgpu_fasta_load(const char *path, uint64_t n_records, uint64_t row_stride, uint8_t pad, uint8_t *out_matrix,
                       uint64_t *out_len, char *out_names, uint64_t *out_name_off);

/* The two text layouts of the distance step, written straight to `path` (host code, no device work): replaces the print
 * loops of distance.py:100-105 (SNPGPU_TSV_PAIRWISE: "Seq1\tSeq2\tDistance" header, one line per ordered pair, the
 * diagonal included) and distance.py:107-114 (SNPGPU_TSV_MATRIX: header "\t" + ids, one row per id).  ids: the names
 * back to back, name i = ids[id_off[i], id_off[i+1]); matrix: HOST int32, row i at matrix + i * row_stride.
 * SNPGPU_E_IO when the file cannot be created or written. */
#define SNPGPU_TSV_PAIRWISE 0
#define SNPGPU_TSV_MATRIX   1
int  snpgpu_write_distance_tsv(const char *path, int layout, const char *ids, const uint64_t *id_off, uint32_t n,
                               const int32_t *matrix, uint64_t row_stride);

/* ---- close pairs and SNP-threshold clusters (csrc/clusters.hip) -------------------------------------------------------
 * Additive entries of ABI 7: they extend what distance.py:93-106 hands the user and change nothing it writes.  The reference
 * prints every ordered pair (distance.py:100-106); these keep the rows with Distance <= T and group the samples that a chain
 * of such pairs joins, on the device, from the matrix snpgpu_distance_packed_dev leaves there.
 *
 * snpgpu_close_pairs_dev: rows [row_lo, row_hi) of the device int32 matrix (row i at d_matrix + i * row_stride elements,
 * row_stride >= n; rows outside the range are never read, so d_matrix may be where row 0 WOULD lie in front of a band of
 * rows; 4-byte aligned) as a CSR of their entries <= threshold over the columns j < n — ascending j, the diagonal included,
 * whatever lies between n and row_stride ignored: d_row_off[row_hi - row_lo + 1], d_col[], d_dist[].  No atomics place the
 * entries: the same matrix gives the same bytes.  *out_n (host) is always set to the number of entries; when it exceeds
 * `capacity` nothing else is written, and capacity 0 only counts.  The call waits for the stream once (the count). */
int  snpgpu_close_pairs_dev(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, uint64_t row_stride, uint32_t row_lo,
                            uint32_t row_hi, int32_t threshold, uint64_t capacity, uint64_t *d_row_off, uint32_t *d_col,
                            int32_t *d_dist, uint64_t *out_n);
/* Host form (as snpgpu_distance, distance.py:93-98): packs the symbols, computes the matrix on the device, thresholds it there
 * and copies only the CSR back — with out_matrix null the n x n matrix never crosses the host link.  out_matrix not null (a
 * caller that writes the reference's two tables as well): the n x n int32 matrix of snpgpu_distance is copied there too, from
 * the same computation, whatever the capacity.  Same capacity protocol for the CSR: a call whose count exceeds `capacity`
 * has computed the matrix for the count alone, and the caller's second call computes it again. */
int  snpgpu_close_pairs(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, int32_t threshold,
                        uint64_t capacity, uint64_t *out_row_off, uint32_t *out_col, int32_t *out_dist, uint64_t *out_n,
                        int32_t *out_matrix);
/* Connected components of the graph of such a CSR over n nodes (d_row_off[n + 1], n_edges entries; one or both directions of
 * an edge, diagonal entries allowed) at every one of n_thresholds thresholds (HOST array) in one call: an entry takes part at
 * threshold t when its distance is <= t.  d_out_numbers[t * n + i] = the cluster number of node i at thresholds[t]: clusters
 * are numbered 1, 2, ... in the order of their smallest node; out_n_clusters[t] (host) = how many.  Min-label hooking and
 * pointer jumping until a round changes nothing (the round count is not bounded in advance; each round waits for the stream). */
int  snpgpu_clusters_dev(snpgpu_ctx *ctx, uint32_t n, const uint64_t *d_row_off, const uint32_t *d_col, const int32_t *d_dist,
                         uint64_t n_edges, const int32_t *thresholds, uint32_t n_thresholds, uint32_t *d_out_numbers,
                         uint32_t *out_n_clusters);
/* Host-array form of snpgpu_clusters_dev; SNPGPU_E_ARG when the offsets do not rise from 0 to n_edges. */
int  snpgpu_clusters(snpgpu_ctx *ctx, uint32_t n, const uint64_t *row_off, const uint32_t *col, const int32_t *dist,
                     uint64_t n_edges, const int32_t *thresholds, uint32_t n_thresholds, uint32_t *out_numbers,
                     uint32_t *out_n_clusters);
/* The two texts (host code, the thread scheme and CPU budget of snpgpu_write_distance_tsv): the close-pairs file is the
 * header and the rows of the pairwise file of distance.py:100-106 that the HOST CSR holds ("id_i\tid_col\tdist\n", row by
 * row); the clusters file is "Id\t" + the thresholds joined by TAB, then one row per id: the id and numbers[t * n + i] for
 * every t.  SNPGPU_E_IO when the file cannot be created or written. */
int  snpgpu_write_close_pairs_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n,
                                  const uint64_t *row_off, const uint32_t *col, const int32_t *dist);
int  snpgpu_write_clusters_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n,
                               const int32_t *thresholds, uint32_t n_thresholds, const uint32_t *numbers);

/* ---- minimum spanning tree and single-linkage dendrogram (csrc/mst.hip) ------------------------------------------------
 * Additive entries of ABI 7, like the ones above.  Samples are 0 ... n-1; edge {i, j}, i < j, weighs matrix[i][j] (signed
 * int32); the edges are totally ordered by (d, i, j) and THE tree is the one Kruskal's algorithm builds in that order, so it
 * is unique: the same matrix gives the same bytes.  For any T its edges with d <= T have the components snpgpu_clusters
 * reports at T.
 *
 * snpgpu_mst_dev: the minimum spanning forest of the entries of rows [row_lo, row_hi) of the device matrix, addressed as for
 * snpgpu_close_pairs_dev (row i at d_matrix + i * row_stride, rows outside the range never read, columns >= n and the diagonal
 * never taken as edges, whatever they hold).  d_u[], d_v[], d_dist[] (room for n - 1 each) receive the edges in ascending
 * (d, u, v), u < v; *out_n_edges and *out_rounds (host) how many there are and how many Boruvka rounds picked them, at most
 * ceil(log2 n).  An empty range or n <= 1: 0 edges, 0 rounds.  The call waits for the stream once per round. */
int  snpgpu_mst_dev(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, uint64_t row_stride, uint32_t row_lo, uint32_t row_hi,
                    uint32_t *d_u, uint32_t *d_v, int32_t *d_dist, uint32_t *out_n_edges, uint32_t *out_rounds);
/* Host form (as snpgpu_close_pairs): packs the symbols, computes the matrix and builds the tree on the device; out_u, out_v,
 * out_dist hold n_rows - 1 edges.  With out_matrix null the n x n matrix never crosses the host link; not null: it is copied
 * there too, from the same computation. */
int  snpgpu_mst(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, uint32_t *out_u, uint32_t *out_v,
                int32_t *out_dist, int32_t *out_matrix);
/* snpgpu_mst and, with want_pairs not 0, snpgpu_close_pairs (same threshold / capacity protocol, same outputs) from ONE
 * computation of the matrix: for a caller that writes the tree next to the close pairs or the clusters. */
int  snpgpu_mst_close_pairs(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, uint32_t *out_u,
                            uint32_t *out_v, int32_t *out_dist, int32_t *out_matrix, int want_pairs, int32_t threshold,
                            uint64_t capacity, uint64_t *out_row_off, uint32_t *out_col, int32_t *out_pair_dist, uint64_t *out_n);
/* Host code: Kruskal in the order (d, min(u,v), max(u,v)) over an edge list on n nodes — duplicates and either orientation of
 * an edge allowed —, which merges the forests that several ranks found in their bands.  out_u / out_v / out_dist: room for
 * min(n_edges, n - 1); a disconnected list gives a forest.  SNPGPU_E_ARG for an index >= n or u == v. */
int  snpgpu_mst_of_edges(uint32_t n, const uint32_t *u, const uint32_t *v, const int32_t *dist, uint64_t n_edges,
                         uint32_t *out_u, uint32_t *out_v, int32_t *out_dist, uint32_t *out_n);
/* The two texts (host code).  MST file: "Seq1\tSeq2\tDistance\n", then "id_u\tid_v\td\n" per edge as given.  Dendrogram: one
 * Newick line.  The edges, which must be a spanning tree of the n samples in ascending (d, i, j) with d >= 0 (else
 * SNPGPU_E_ARG), are taken in order; each joins the groups of its ends under a node of height d / 2 (leaves: 0), the child
 * with the smaller sample first; a branch length is (d_parent - d_child) / 2 written from the integer ("7" or "7.5"), the root
 * has none; an id that is not [A-Za-z0-9.|-]+ is put in single quotes with every ' doubled.  n = 0: ";\n", n = 1: "id;\n".
 * No recursion.  SNPGPU_E_IO when the file cannot be created or written. */
int  snpgpu_write_mst_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *u,
                          const uint32_t *v, const int32_t *dist, uint32_t n_edges);
int  snpgpu_write_dendrogram_newick(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *u,
                                    const uint32_t *v, const int32_t *dist, uint32_t n_edges);

/* ---- complete- and average-linkage trees (csrc/linkage.hip) ---------------------------------------------------------------
 * Additive entries of ABI 7, like the ones above.  Samples are 0 ... n-1.  A cluster is a set of samples, its id its smallest
 * sample.  kind 0, complete linkage: d(A,B) = max d(a,b); kind 1, average linkage (UPGMA): d(A,B) = S(A,B) / (|A| |B|), S the
 * sum of d(a,b), held as the integer S and the two sizes, never as a float.  Pairs of live clusters are totally ordered by
 * (d(A,B), min id, max id), rationals compared exactly; THE tree is the one that merges the least pair n - 1 times, so it is
 * unique and its merges (a, b, sizeA, sizeB, num), a = idA < b = idB, num = d (complete) or S (average), ascend in that key.
 *
 * snpgpu_linkage_dev: the tree of the symmetric device int32 matrix (row i at d_matrix + i * row_stride elements, row_stride >= n,
 * 4-byte aligned; columns >= n and the diagonal are never taken, whatever they hold; the matrix is not modified).  d_a, d_b,
 * d_size_a, d_size_b, d_num (room for n - 1 each) receive the merges in ascending key order; *out_n_merges and *out_rounds
 * (host) how many there are and how many rounds built them: a round merges every reciprocal-nearest-neighbour pair, so there
 * are at most n - 1.  n <= 1: 0 merges, 0 rounds.  Every comparison is exact: products of two 64-bit numbers are compared in
 * 128 bits.  A matrix whose sums could leave 64 bits — (largest entry) * floor(n/2) * ceil(n/2) >= 2^64, average linkage only —
 * and a matrix with a negative entry are refused with SNPGPU_E_ARG before the first round.  Needs 8 n^2 bytes of device memory
 * (SNPGPU_E_NOMEM).  The call waits for the stream once per round; the final ordering is host code. */
int  snpgpu_linkage_dev(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, uint64_t row_stride, int kind, uint32_t *d_a,
                        uint32_t *d_b, uint32_t *d_size_a, uint32_t *d_size_b, uint64_t *d_num, uint32_t *out_n_merges,
                        uint32_t *out_rounds);
/* Host form (as snpgpu_mst): packs the symbols, computes the matrix and builds the tree on the device; the five host arrays hold
 * n_rows - 1 merges.  With out_matrix null the n x n matrix never crosses the host link; not null: it is copied there too, from
 * the same computation. */
int  snpgpu_linkage(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, int kind, uint32_t *out_a,
                    uint32_t *out_b, uint32_t *out_size_a, uint32_t *out_size_b, uint64_t *out_num, int32_t *out_matrix,
                    uint32_t *out_n_merges, uint32_t *out_rounds);
/* Host form for a caller that has the matrix already (a table was asked for): uploads the HOST int32 matrix and builds the tree. */
int  snpgpu_linkage_of_matrix(snpgpu_ctx *ctx, const int32_t *matrix, uint32_t n, uint64_t row_stride, int kind, uint32_t *out_a,
                              uint32_t *out_b, uint32_t *out_size_a, uint32_t *out_size_b, uint64_t *out_num,
                              uint32_t *out_n_merges, uint32_t *out_rounds);
/* Host code: the clusters of a merge list (ascending key order, as the calls above give it) at every threshold: a merge belongs
 * to T when num <= T (complete) or num <= T * sizeA * sizeB (average); heights are monotone, so those are a prefix.
 * out_numbers[t * n + i] and out_n_clusters[t] as snpgpu_clusters: numbers 1, 2, ... in the order of the smallest sample.  With
 * complete linkage every two members of a cluster are within T.  SNPGPU_E_ARG unless the merges are those of a tree of the n
 * samples, checked as the writers below check them: a < b < n, both live clusters of the sizes given, fewer than n merges. */
int  snpgpu_linkage_cut(int kind, uint32_t n, const uint32_t *a, const uint32_t *b, const uint32_t *size_a, const uint32_t *size_b,
                        const uint64_t *num, uint32_t n_merges, const int32_t *thresholds, uint32_t n_thresholds,
                        uint32_t *out_numbers, uint32_t *out_n_clusters);
/* The two texts (host code).  Merge file: "Seq1\tSeq2\tSize1\tSize2\tDistance\n", then per merge in the order given the ids of a
 * and b, the two sizes and the distance: num for complete linkage; for average linkage S / (sizeA sizeB) rounded half up to
 * exactly six decimals, in integers: (2 S 10^6 + sa sb) / (2 sa sb), split at 10^6.  Dendrogram: one Newick line in the grammar
 * of snpgpu_write_dendrogram_newick (same quoting, the child with the smaller sample first, no length at the root, ";\n" for
 * n = 0, "id;\n" for n = 1, no recursion).  A node's height in integer millionths is round_half_up(num 10^6 / (2 sa sb)), sa sb
 * taken as 1 for complete linkage, leaves 0; a branch length is H_parent - H_child: the integer part, then, when the fraction is
 * not zero, "." and its six digits without trailing zeros ("7", "7.5", "0.0625").  SNPGPU_E_ARG unless the merges are a tree
 * of the n samples: a < b < n live clusters of the sizes given, n - 1 of them for the dendrogram, heights that do not fall —
 * and when a distance does not fit 64 bits as millionths (num 10^6 / (sa sb) >= 2^64: the dendrogram of either kind, the merge
 * file of average linkage; no sum of int32 entries comes near it). */
int  snpgpu_write_linkage_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, int kind, const uint32_t *a,
                              const uint32_t *b, const uint32_t *size_a, const uint32_t *size_b, const uint64_t *num,
                              uint32_t n_merges);
int  snpgpu_write_linkage_newick(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, int kind,
                                 const uint32_t *a, const uint32_t *b, const uint32_t *size_a, const uint32_t *size_b,
                                 const uint64_t *num, uint32_t n_merges);

/* ---- neighbour-joining tree (csrc/nj.hip) ------------------------------------------------------------------------------------
 * Additive entries of ABI 7, like the ones above: the standard distance-based phylogeny (Saitou & Nei's method with the
 * Studier-Keppler criterion), which assumes no molecular clock and on an additive matrix returns the true tree with its branch
 * lengths.  In floating point the method depends on summation order and breaks ties by rounding noise; here it is stated in
 * integers, in fixed point, so every sum is associative, any reduction order gives the same value and THE tree is unique.
 *
 * Samples are 0 ... n-1.  F = 20 fractional bits; working values are w(i,k) = matrix[i][k] << F, signed 64 bits.  A node lives
 * in a slot; slot i starts as sample i and a joined node keeps the smaller of its two slots, so a node's slot is its smallest
 * sample.  r is the number of live slots.  While r > 3, one round: R(i) = the sum of w(i,k) over live k != i; for live i < j,
 * Q(i,j) = (r-2) w(i,j) - R(i) - R(j); the pair that is least in the order (Q, i, j), call it a < b, is joined with the branch
 * lengths La = floor(((r-2) w(a,b) + R(a) - R(b)) / (2 (r-2))) (towards minus infinity) and Lb = w(a,b) - La; the new node takes
 * slot a, and for every other live k, w(a,k) = w(k,a) = floor((w(a,k) + w(b,k) - w(a,b)) / 2); slot b retires; the record is
 * (a, b, La, Lb).  Lengths and distances may be negative and are kept as they are: nothing is clamped.  The last three live
 * slots a < b < c are the star: La = floor((w(a,b) + w(a,c) - w(b,c)) / 2), Lb = w(a,b) - La, Lc = w(a,c) - La.  n = 2: the star
 * is (0, 1, none) with L0 = floor(w / 2), L1 = w - L0.  n <= 1: nothing.  So there are max(n - 3, 0) merges, in round order
 * (nothing is sorted afterwards), and at most one star.  The floors cost at most 2^-20 SNP per level of the tree.
 *
 * Range: with L = floor(2^61 / max(n, 1)), every |Q| stays below 2^63 while every |w| <= L.  A matrix that holds a negative
 * entry, or whose (largest entry) << F exceeds L, is refused with SNPGPU_E_ARG before the first round and before any record is
 * written (n beyond 1024 at entries of 2^31 - 1; at 10 000 samples entries up to 219 million pass).  A sticky device flag is
 * raised when a round produces a |w| above L; it is read once after the last round, and then the call returns SNPGPU_E_ARG and
 * the outputs are unspecified.  In the Python statement of the tests no random, tied, planted or additive matrix grew beyond its
 * initial largest value, so that flag is a guard no test reaches on the device.
 *
 * snpgpu_nj_dev: the tree of the symmetric device int32 matrix (row i at d_matrix + i * row_stride elements, row_stride >= n,
 * 4-byte aligned; the diagonal and columns >= n are never read; the matrix is not modified).  d_a, d_b (uint32), d_len_a,
 * d_len_b (int64), room for n - 3 each (may be null for n <= 3), receive the merges; out_star[3] (host; 0xFFFFFFFF for none),
 * out_star_len[3] (host) the star; *out_n_merges (host) the number of merges.  All n - 3 rounds are enqueued on the context's
 * stream without a host wait in between: the call waits once before the first round, for the refusal, and once at the end, for the
 * star and the flag.  Needs 8 n^2 bytes of device memory, the n x n working matrix (SNPGPU_E_NOMEM): when an eighth of the stored
 * slots have retired the live columns of every row are moved together in place, in their order. */
int  snpgpu_nj_dev(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n, uint64_t row_stride, uint32_t *d_a, uint32_t *d_b,
                   int64_t *d_len_a, int64_t *d_len_b, uint32_t *out_star, int64_t *out_star_len, uint32_t *out_n_merges);
/* Host form (as snpgpu_linkage): packs the symbols, computes the matrix and builds the tree on the device; the four host arrays
 * hold n_rows - 3 merges.  With out_matrix null the n x n matrix never crosses the host link; not null: it is copied there too,
 * from the same computation. */
int  snpgpu_nj(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, uint32_t *out_a, uint32_t *out_b,
               int64_t *out_len_a, int64_t *out_len_b, int32_t *out_matrix, uint32_t *out_star, int64_t *out_star_len,
               uint32_t *out_n_merges);
/* Host form for a caller that has the matrix already (a table was asked for): uploads the HOST int32 matrix and builds the tree. */
int  snpgpu_nj_of_matrix(snpgpu_ctx *ctx, const int32_t *matrix, uint32_t n, uint64_t row_stride, uint32_t *out_a, uint32_t *out_b,
                         int64_t *out_len_a, int64_t *out_len_b, uint32_t *out_star, int64_t *out_star_len,
                         uint32_t *out_n_merges);
/* The text (host code): one Newick line in the grammar of snpgpu_write_linkage_newick / snpgpu_write_dendrogram_newick (same
 * quoting of ids, no recursion).  Inside a node the child whose smallest sample is smaller comes first; the star is a
 * trifurcation at the top, "(A:la,B:lb,C:lc);\n", its three children in the same order; n = 2: "(id0:l0,id1:l1);\n"; n = 1:
 * "id;\n"; n = 0: ";\n".  A length x is written from integer millionths m = floor((2 x 10^6 + 2^F) / 2^(F+1)), computed in 128
 * bits (half up): "-" when m < 0, the integer part of |m|, then, when the fraction is not zero, "." and its six digits without
 * trailing zeros ("7", "7.5", "-0.0625", "0").  SNPGPU_E_ARG unless the records are a tree of the n samples: a < b < n, both
 * live, max(n - 3, 0) merges, and a star of exactly the live slots that are left, ascending.  SNPGPU_E_IO when the file cannot be
 * created or written. */
int  snpgpu_write_nj_newick(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *a,
                            const uint32_t *b, const int64_t *len_a, const int64_t *len_b, uint32_t n_merges,
                            const uint32_t *star, const int64_t *star_len);

/* ---- bootstrap support of the neighbour-joining tree (csrc/nj_bootstrap.hip) ------------------------------------------------
 * Additive entries of ABI 7, like the ones above: Felsenstein's bootstrap of the tree above, which of its branches the data
 * supports.  Because the tree is stated in integers with a pinned tie-break, every replicate tree is unique and so are the
 * counts: the support values are pinned byte for byte (tests/nj_bootstrap_cases.py restates all of this in Python).
 *
 * Samples are the rows 0 ... n-1, s the column count, B >= 1 the number of replicates, seed a 64-bit unsigned integer.  All
 * arithmetic modulo 2^64:
 *   G       = 0x9E3779B97F4A7C15
 *   mix(z)  : z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *   draw(seed, b, k) = mix(mix(seed + G (b + 1)) + G (k + 1))       replicate b = 0 ... B-1, position k = 0 ... s-1
 *   c(b, k)          = floor(draw(seed, b, k) s / 2^64)             the high half of the 64 x 64-bit product
 * Replicate b: its matrix is the distance over the multiset of columns {c(b,k)}: D_b(i,j) = the number of k at which both bytes
 * of column c(b,k) are in ACGT after upper-casing and differ (the order of the columns does not enter); its tree is the
 * neighbour-joining tree of D_b exactly as stated above.  A replicate the range guard refuses makes the whole call fail alike.
 * Bipartitions: a tree of n >= 4 samples has n - 3 join records (a_t, b_t); record t defines the leaf set under the new node.
 * Its canonical form is the side that does NOT hold sample 0 (the complement within the n samples when the leaf set holds it):
 * n - 3 distinct non-trivial bipartitions per tree, each a bitset of W = ceil(n / 64) 64-bit words, bit i of word i / 64 sample
 * i, bits >= n zero.  Support(t) of the main tree (of the unresampled matrix) is the number of replicates whose tree holds main
 * bipartition t, 0 ... B; Percent(t) = floor((200 Support(t) + B) / (2 B)), half up, in integers.  n <= 3: nothing to count.
 *
 * snpgpu_bootstrap_columns_dev: d_cols[n_sites] (uint32) = c(replicate, .) in draw order.
 * snpgpu_resample_packed_dev: d_out = the pack of sym[:, cols] from d_packed, the pack of sym (snpgpu_pack_matrix_dev: n_rows
 * rows of snpgpu_packed_row_bytes(n_sites) bytes); d_out has rows of snpgpu_packed_row_bytes(n_cols) bytes and comes out
 * byte-identical to snpgpu_pack_matrix_dev of the gathered symbols: all four planes, padding bits and words zero.  Any list,
 * any order; a sorted one reads best.  The call first waits for the largest index of the list: one >= n_sites is refused with
 * SNPGPU_E_ARG before anything is written.
 * snpgpu_nj_splits_dev: from the device join records of n_trees trees of n samples (tree i at d_a / d_b + i (n - 3)),
 * d_out[n_trees][n - 3][W] (uint64) in canonical form; n W words of workspace per tree are allocated (SNPGPU_E_NOMEM).  A record
 * that names a slot >= n gives a zero row.  Nothing is written for n <= 3.
 * snpgpu_split_support_dev: d_counts[i] = the number of the n_rep rows of d_rep equal to row i of d_main, on all n_words words;
 * the n_main rows of d_main are distinct (equal ones: one of them gets the count).  No hash: the rows' indices are sorted by
 * their words and every other row is looked up in that order. */
int  snpgpu_bootstrap_columns_dev(snpgpu_ctx *ctx, uint64_t seed, uint32_t replicate, uint32_t n_sites, uint32_t *d_cols);
/* ... the same columns ascending, as the host form below hands them to the resample: the draws and the library's merge sort in a
 * workspace of its own (3 n_sites words), copied to d_cols; waits for the stream. */
int  snpgpu_bootstrap_columns_sorted_dev(snpgpu_ctx *ctx, uint64_t seed, uint32_t replicate, uint32_t n_sites, uint32_t *d_cols);
int  snpgpu_resample_packed_dev(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, const uint32_t *d_cols,
                                uint32_t n_cols, void *d_out);
int  snpgpu_nj_splits_dev(snpgpu_ctx *ctx, const uint32_t *d_a, const uint32_t *d_b, uint32_t n, uint32_t n_trees, uint64_t *d_out);
int  snpgpu_split_support_dev(snpgpu_ctx *ctx, const uint64_t *d_main, uint32_t n_main, const uint64_t *d_rep, uint64_t n_rep,
                              uint32_t n_words, uint32_t *d_counts);
/* Host form on symbols: the outputs of snpgpu_nj, then out_support[n_rows - 3] (may be null for n_rows <= 3), the counts of the
 * main tree's joins in round order.  replicates == 0 and null outputs are refused (SNPGPU_E_ARG) before any output is written.
 * One upload and pack; per replicate the columns, their sort, the resample, the distance kernel and the NJ rounds, into one
 * resampled pack and one n x n matrix; 8 bytes per join and replicate stay on the device; bipartitions and counts run over the
 * replicates in bands sized from the free device memory.  Only the main tree and the counts cross the host link. */
int  snpgpu_nj_bootstrap(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, uint32_t replicates,
                         uint64_t seed, uint32_t *out_a, uint32_t *out_b, int64_t *out_len_a, int64_t *out_len_b,
                         int32_t *out_matrix, uint32_t *out_star, int64_t *out_star_len, uint32_t *out_n_merges,
                         uint32_t *out_support);
/* The text (host code).  snpgpu_write_nj_newick_support: the line of snpgpu_write_nj_newick with the node of merge e carrying
 * Percent(e) as a decimal integer between its ")" and its ":", "((s1:1,s2:2)87:0.5,...);"; the trifurcation at the top carries
 * none, so with n <= 3 the file is that of snpgpu_write_nj_newick.  snpgpu_write_nj_support: a table, header
 * "Seq1\tSeq2\tSize\tSupport\tReplicates", one row per join in round order: the ids of slots a and b, the number of leaves
 * under the new node, the count, B.  SNPGPU_E_ARG also for replicates == 0, a null support array beside a merge, a count above
 * the replicates. */
int  snpgpu_write_nj_newick_support(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *a,
                                    const uint32_t *b, const int64_t *len_a, const int64_t *len_b, uint32_t n_merges,
                                    const uint32_t *star, const int64_t *star_len, const uint32_t *support, uint32_t replicates);
int  snpgpu_write_nj_support(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *a,
                             const uint32_t *b, uint32_t n_merges, const uint32_t *support, uint32_t replicates);

/* ---- the differing sites of pairs (csrc/pair_sites.hip) -----------------------------------------------------------------
 * Additive entries of ABI 7, like the ones above: by which columns two samples differ.  Column s of pair (a, b) differs iff
 * both bytes, after upper-casing, are in {A,C,G,T} and are not equal (utils.py:1135-1165, what the distance kernel counts), so
 * pair (a, b) has matrix[a][b] entries.  A pair's entries come in ascending column order, the pairs in the order given.
 *
 * snpgpu_pair_sites_dev: d_packed is the packed matrix of snpgpu_pack_matrix_dev (rows of snpgpu_packed_row_bytes(n_sites)
 * bytes, 16-byte aligned), d_a / d_b device lists of n_pairs row indices: any order, duplicates allowed, a == b gives no
 * entries.  d_pair_off[n_pairs + 1] receives the offsets, d_site[] the 0-based columns, d_bases[] one byte per entry: the low
 * nibble is the first sample (bits 0-1 the base A0 C1 G2 T3, bit 2 lower case), the high nibble the second.  No atomic decides
 * a position: the same input gives the same bytes.  The capacity protocol of snpgpu_close_pairs_dev: *out_n (host) is always
 * set; when it exceeds `capacity` nothing else is written; capacity 0 only counts; the call waits for the stream once, for the
 * count.  SNPGPU_E_ARG, with *out_n 0 and nothing written, when a pair names a row >= n_rows or the entries of the call reach 2^32. */
int  snpgpu_pair_sites_dev(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, const uint32_t *d_a,
                           const uint32_t *d_b, uint64_t n_pairs, uint64_t capacity, uint64_t *d_pair_off, uint32_t *d_site,
                           uint8_t *d_bases, uint64_t *out_n);
/* Host form: uploads and packs the symbols (as snpgpu_distance), uploads the lists, calls the above and copies the three
 * arrays back.  The indices are checked on the host. */
int  snpgpu_pair_sites(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, const uint32_t *a,
                       const uint32_t *b, uint64_t n_pairs, uint64_t capacity, uint64_t *out_pair_off, uint32_t *out_site,
                       uint8_t *out_bases, uint64_t *out_n);
/* Everything the distance step hands out from ONE upload, pack and computation of the matrix: snpgpu_mst_close_pairs with the
 * tree optional as well (want_tree 0: out_u / out_v / out_dist are not touched) and, with keep_packed not 0, the packed matrix
 * left in the context — where snpgpu_pair_sites_kept, the host form above without symbols, finds it for any number of pair
 * lists (the tree's edges, the close pairs: their entries are the sum of the distances the first call returned, so the caller
 * knows the capacity) until snpgpu_packed_drop, the next keeping call or the end of the context frees it. */
int  snpgpu_distance_outputs(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, int want_tree,
                             uint32_t *out_u, uint32_t *out_v, int32_t *out_dist, int32_t *out_matrix, int want_pairs,
                             int32_t threshold, uint64_t capacity, uint64_t *out_row_off, uint32_t *out_col,
                             int32_t *out_pair_dist, uint64_t *out_n, int keep_packed);
int  snpgpu_pair_sites_kept(snpgpu_ctx *ctx, const uint32_t *a, const uint32_t *b, uint64_t n_pairs, uint64_t capacity,
                            uint64_t *out_pair_off, uint32_t *out_site, uint8_t *out_bases, uint64_t *out_n);
int  snpgpu_packed_drop(snpgpu_ctx *ctx);
/* The text (host code, the thread scheme and CPU budget of snpgpu_write_distance_tsv; the threads take equal shares of the
 * entries, not of the pairs): one row per entry of HOST arrays as the calls above fill them.  Without a site table (the last four
 * arguments null): "Seq1\tSeq2\tSite\tBase1\tBase2\n", then "id_a\tid_b\t<1-based column>\t<letter>\t<letter>\n".  With one —
 * chrom_names / chrom_off the contig names and their offsets, chrom_of_site[] / pos_of_site[] the contig and position of every
 * column of the matrix (the caller's: no `site` may lie outside them) —: "Seq1\tSeq2\tChrom\tPos\tBase1\tBase2\n" and the
 * contig name and position in place of the column.  Letters keep their case; a pair without entries has no row.
 * SNPGPU_E_ARG for an index >= n or offsets that do not rise from 0; SNPGPU_E_IO when the file cannot be created or written. */
int  snpgpu_write_pair_sites_tsv(const char *path, const char *ids, const uint64_t *id_off, uint32_t n, const uint32_t *a,
                                 const uint32_t *b, uint64_t n_pairs, const uint64_t *pair_off, const uint32_t *site,
                                 const uint8_t *bases, const char *chrom_names, const uint64_t *chrom_off,
                                 const uint32_t *chrom_of_site, const uint64_t *pos_of_site);

/* ---- query-against-database nearest neighbours (csrc/nearest.hip) --------------------------------------------------------
 * Additive entries of ABI 7, like the ones above: q query samples against n database samples, without the (n + q)^2 matrix.
 * d(i, j) counts the columns at which query i and database sample j differ under the predicate of the distance kernel
 * (utils.py:1135-1165).  For query i the database samples with d(i, j) <= threshold are ordered by (d, j) and the first k kept
 * (k = 0: all of them; threshold = INT32_MAX: none): ties at the cut go to the smaller database index, so the answer is unique.
 *
 * snpgpu_distance_rect_packed_dev: d_packed_q (q rows) and d_packed_db (n rows) are packed matrices of snpgpu_pack_matrix_dev
 * over the same n_sites (rows of snpgpu_packed_row_bytes(n_sites) bytes, 16-byte aligned); d_out[i * out_stride + j] = d(i, j)
 * for i < q, j < n (int32, out_stride >= n elements, 4-byte aligned).  Nothing is written beyond column n of a row or beyond
 * row q.  route: 0 auto (narrow for q <= 64, the measured crossover), 1 narrow (tiles of 16 queries x 64 database rows: the
 * sweep of the database is HBM-bound for few queries), 2 tile (128 x 128, the shape of snpgpu_distance_packed_dev: VALU-bound);
 * both give the same numbers.  With fewer tiles than CUs and at least 4 slabs per row (slabs of 16 words narrow, 4 words tile)
 * the word range is split and the parts add into the zeroed output with integer atomics.  Enqueued on the context's stream;
 * nothing waits. */
int  snpgpu_distance_rect_packed_dev(snpgpu_ctx *ctx, const void *d_packed_q, uint32_t q, const void *d_packed_db, uint32_t n,
                                     uint32_t n_sites, int route, int32_t *d_out, uint64_t out_stride);
/* snpgpu_nearest_dev: the selection over rows 0 ... q-1 of a device int32 matrix (row i at d_matrix + i * row_stride elements,
 * row_stride >= n, 4-byte aligned; signed entries; whatever lies between n and row_stride is never read) as a CSR:
 * d_row_off[q + 1], then d_col[] / d_dist[] with row i's entries in ascending (d, column).  A radix select finds the k-th
 * smallest value of a row that k cuts; every position comes from prefix sums and a stable sort, none from an atomic: the same
 * matrix gives the same bytes.  The capacity protocol of snpgpu_close_pairs_dev: *out_n (host) is always set to the number of
 * entries; when it exceeds `capacity` nothing else is written, and capacity 0 only counts.  q = 0 or n = 0: no entries, the
 * offsets (written when capacity is not 0) all zero.  The call waits for the stream for the count, and again before it frees
 * its sort workspace. */
int  snpgpu_nearest_dev(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t q, uint32_t n, uint64_t row_stride, uint32_t k,
                        int32_t threshold, uint64_t capacity, uint64_t *d_row_off, uint32_t *d_col, int32_t *d_dist,
                        uint64_t *out_n);
/* Host form: uploads and packs both symbol matrices (q x n_sites and n x n_sites bytes) once, then works through the queries
 * in bands of band_rows rows (0: the largest band whose band x n x 4 bytes stay within a quarter of the free device memory):
 * per band one sweep of the database by snpgpu_distance_rect_packed_dev and one selection.  Queries are independent, so the
 * band size does not change a byte.  Only the CSR crosses the host link — and, with out_matrix not null, the q x n int32
 * matrix (row pitch n).  *out_n is always set; when it exceeds `capacity` (capacity 0 only counts) the contents of the three
 * arrays are unspecified: q * min(k, n) entries always suffice when k is not 0. */
int  snpgpu_nearest(snpgpu_ctx *ctx, const uint8_t *q_symbols, uint32_t q, const uint8_t *db_symbols, uint32_t n,
                    uint32_t n_sites, uint32_t k, int32_t threshold, uint32_t band_rows, int route, uint64_t capacity,
                    uint64_t *out_row_off, uint32_t *out_col, int32_t *out_dist, uint64_t *out_n, int32_t *out_matrix);
/* The text (host code, the thread scheme and CPU budget of snpgpu_write_distance_tsv; the threads take equal shares of the
 * entries): "Seq1\tSeq2\tDistance\n", then "query_id\tdb_id\td\n" per entry of the HOST CSR, query by query in its order.
 * SNPGPU_E_ARG for a column >= n or offsets that do not rise from 0; SNPGPU_E_IO when the file cannot be created or written. */
int  snpgpu_write_nearest_tsv(const char *path, const char *q_ids, const uint64_t *q_id_off, uint32_t q, const char *db_ids,
                              const uint64_t *db_id_off, uint32_t n, const uint64_t *row_off, const uint32_t *col,
                              const int32_t *dist);

/* ---- compared-site counts (csrc/compared.hip) ------------------------------------------------------------------------------
 * Additive entries of ABI 7, like the ones above: at how many columns a pair was compared at all.  Compared(i, j) counts the
 * columns at which both bytes, after upper-casing a-z, are in {A,C,G,T} — the predicate of the distance kernel
 * (utils.py:1135-1165) without "and differ" — so Distance(i, j) <= Compared(i, j) <= min(Compared(i, i), Compared(j, j)),
 * Compared(i, i) is sample i's own count of ACGT columns, and the matrix is symmetric.  int32, as the distance.
 *
 * snpgpu_valid_plane_dev: the `valid` words of the packed matrix of snpgpu_pack_matrix_dev (n_rows rows of
 * snpgpu_packed_row_bytes(n_sites) bytes) as a dense plane: one uint32 per 32 sites, bit i of word w = column 32 w + i, row r at
 * d_plane + r * snpgpu_valid_plane_row_bytes(n_sites) bytes — rows are padded to a multiple of 16 words (64 bytes).  Every byte of
 * the n_rows rows is written, the padding words zero whatever lay there, and nothing behind the last row; no bit at or beyond
 * n_sites is set whatever the packed matrix holds.  Both pointers 16-byte aligned.  n_rows or n_sites 0: nothing to do.
 * Enqueued on the context's stream; nothing waits. */
size_t snpgpu_valid_plane_row_bytes(uint32_t n_sites);
int  snpgpu_valid_plane_dev(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, void *d_plane);
/* snpgpu_compared_rect_dev: d_plane_q (q rows) and d_plane_db (n rows) are planes of snpgpu_valid_plane_dev over the same
 * n_sites; d_out[i * out_stride + j] = Compared(query i, database sample j) for i < q, j < n (int32, out_stride >= n elements,
 * 4-byte aligned) — the conventions of snpgpu_distance_rect_packed_dev: nothing is written beyond column n of a row or beyond
 * row q.  The same plane twice with q == n is the symmetric matrix: the tiles of the upper triangle are computed and mirrored.
 * Tiles of 128 x 128 pairs, no split of the word range for shapes of few tiles.  n_sites == 0 gives zeros.  Enqueued on the
 * context's stream; nothing waits. */
int  snpgpu_compared_rect_dev(snpgpu_ctx *ctx, const void *d_plane_q, uint32_t q, const void *d_plane_db, uint32_t n,
                              uint32_t n_sites, int32_t *d_out, uint64_t out_stride);
/* snpgpu_compared_pairs_dev: d_out[p] = Compared(row d_a[p] of plane a, row d_b[p] of plane b) for the n_pairs pairs of two
 * device lists (any order, duplicates allowed; d_plane_b may be d_plane_a), without the matrix.  No atomic: the same input gives
 * the same bytes.  SNPGPU_E_ARG, with nothing written, when a pair names a row >= n_a or >= n_b: the lists are checked first,
 * and the call waits for the stream once, for that check. */
int  snpgpu_compared_pairs_dev(snpgpu_ctx *ctx, const void *d_plane_a, uint32_t n_a, const void *d_plane_b, uint32_t n_b,
                               uint32_t n_sites, const uint32_t *d_a, const uint32_t *d_b, uint64_t n_pairs, int32_t *d_out);
/* Host forms: upload and pack the symbols (as snpgpu_distance), extract the plane, call the above and copy the result back.
 * snpgpu_compared: the n x n matrix (row pitch n).  snpgpu_compared_pairs: out[p] for host lists over symbols_a (n_a x n_sites)
 * and symbols_b (n_b x n_sites); a null symbols_b means both indices address symbols_a (n_b is ignored).  The indices are
 * checked on the host: SNPGPU_E_ARG with nothing written. */
int  snpgpu_compared(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n, uint32_t n_sites, int32_t *out_matrix);
int  snpgpu_compared_pairs(snpgpu_ctx *ctx, const uint8_t *symbols_a, uint32_t n_a, const uint8_t *symbols_b, uint32_t n_b,
                           uint32_t n_sites, const uint32_t *a, const uint32_t *b, uint64_t n_pairs, int32_t *out);
/* The text of pair lists with their counts (host code, the thread scheme and CPU budget of snpgpu_write_distance_tsv):
 * "Seq1\tSeq2\tDistance\tCompared\n", then "id_a\tid_b\tdist\tcompared\n" per entry of the HOST arrays a[], b[], dist[],
 * compared[] in the order given; a[] indexes the first id table (n_a ids), b[] the second (n_b ids; the same table may be given
 * twice).  SNPGPU_E_ARG for an index outside its table or 2^32 rows and more; SNPGPU_E_IO when the file cannot be created or
 * written. */
int  snpgpu_write_pair_rows_tsv(const char *path, const char *a_ids, const uint64_t *a_id_off, uint32_t n_a, const char *b_ids,
                                const uint64_t *b_id_off, uint32_t n_b, const uint32_t *a, const uint32_t *b,
                                const int32_t *dist, const int32_t *compared, uint64_t n_rows);

/* ---- per-site allele counts and cluster-defining SNPs (csrc/cluster_snps.hip) --------------------------------------------
 * Additive entries of ABI 7.  A byte is a base iff, after upper-casing, it is one of ACGT (the distance's predicate); the bases
 * are numbered A0 C1 G2 T3.  d_packed is the packed matrix of snpgpu_pack_matrix_dev (rows of snpgpu_packed_row_bytes(n_sites)
 * bytes, 16-byte aligned); every call reads it once.
 *
 * snpgpu_site_counts_dev: d_counts[4 s + b] (int32) = the rows that hold base b at column s, in either case; exactly 4 n_sites
 * elements are written (n_rows - their sum is what a column holds besides bases).  n_rows == 0 gives zeros, n_sites == 0
 * nothing.  Integer atomic adds into the counts: the sums do not depend on their order.  Enqueued on the context's stream;
 * nothing waits.  (The host form is not called snpgpu_site_counts: that is the per-position record of the call kernels.) */
int  snpgpu_site_counts_dev(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, int32_t *d_counts);
/* Host form: uploads and packs the symbols (as snpgpu_distance), calls the above and copies the counts back. */
int  snpgpu_site_counts_host(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, int32_t *out_counts);
/* snpgpu_cluster_snps_dev: d_labels[n_rows] names every row's cluster, 1 ... n_clusters (a number without rows is legal).
 * (cluster c, column s, base b) is an entry iff at least one member of c holds b at s, no member holds another base there
 * (members without a base at s are allowed), and no row outside c holds b at s.  The entries come by cluster ascending, then
 * column ascending — at most four clusters have an entry at a column —: d_cluster_off[n_clusters + 1] (uint64) the offsets of
 * the clusters, d_site[] the 0-based columns, d_base[] 0..3, d_members[] how many members of the cluster hold the base.  No
 * atomic decides a position or an order-dependent value: the same input gives the same bytes.  The capacity protocol of
 * snpgpu_pair_sites_dev: *out_n (host) is always set; when it exceeds `capacity` nothing else is written; capacity 0 only
 * counts.  The call waits for the stream: for the check of the labels, for the count, and at its end (it frees its workspace).
 * SNPGPU_E_ARG, with *out_n 0 and nothing written, when a label is 0 or above n_clusters.  n_rows == 0, n_sites == 0 and
 * n_clusters == 0 are legal and give no entry. */
int  snpgpu_cluster_snps_dev(snpgpu_ctx *ctx, const void *d_packed, uint32_t n_rows, uint32_t n_sites, const uint32_t *d_labels,
                             uint32_t n_clusters, uint64_t capacity, uint64_t *d_cluster_off, uint32_t *d_site, uint8_t *d_base,
                             uint32_t *d_members, uint64_t *out_n);
/* Host form: one upload and pack of the symbols, one count of the sites, then one labelling after another: labels[t][n_rows]
 * with n_clusters[t] clusters, t < n_labellings.  The entries of the labellings follow one another; out_cluster_off holds
 * n_clusters[t] + 1 offsets per labelling, one block after another, each counting from the first entry of the call (so a
 * block's first offset is the number of entries before its labelling).  The capacity protocol above over the sum; the labels
 * are checked on the host. */
int  snpgpu_cluster_snps(snpgpu_ctx *ctx, const uint8_t *symbols, uint32_t n_rows, uint32_t n_sites, const uint32_t *labels,
                         const uint32_t *n_clusters, uint32_t n_labellings, uint64_t capacity, uint64_t *out_cluster_off,
                         uint32_t *out_site, uint8_t *out_base, uint32_t *out_members, uint64_t *out_n);
/* The text (host code).  snpgpu_write_site_counts_tsv: "Site\tA\tC\tG\tT\tOther\n", then per column its 1-based number, the
 * four counts[4 s + b] and n_rows minus their sum.  With a site table (chrom_names / chrom_off / chrom_of_site / pos_of_site as
 * for snpgpu_write_pair_sites_tsv, one entry per column): "Chrom\tPos\tA\tC\tG\tT\tOther\n" and the contig name and position in
 * place of the number.  SNPGPU_E_ARG when a column's counts are negative or sum to more than n_rows.
 * snpgpu_write_cluster_snps_tsv: the HOST arrays of snpgpu_cluster_snps with thresholds[t] naming labelling t and
 * sizes[] holding the sizes of the clusters, n_clusters[t] per labelling, one block after another:
 * "Threshold\tCluster\tSite\tBase\tMembers\tSize\n", then per entry the threshold, the 1-based cluster, the 1-based column (or,
 * with a site table, Chrom and Pos), the base as an upper-case letter, the members and the size.  n_sites: the columns of the
 * matrix; SNPGPU_E_ARG for a site at or above it, a base above 3 or offsets that do not rise from 0.  SNPGPU_E_IO when the file
 * cannot be created or written. */
int  snpgpu_write_site_counts_tsv(const char *path, const int32_t *counts, uint32_t n_sites, uint32_t n_rows, const char *chrom_names,
                                  const uint64_t *chrom_off, const uint32_t *chrom_of_site, const uint64_t *pos_of_site);
int  snpgpu_write_cluster_snps_tsv(const char *path, const int32_t *thresholds, const uint32_t *n_clusters, uint32_t n_labellings,
                                   const uint64_t *cluster_off, const uint32_t *sizes, const uint32_t *site, const uint8_t *base,
                                   const uint32_t *members, uint32_t n_sites, const char *chrom_names, const uint64_t *chrom_off,
                                   const uint32_t *chrom_of_site, const uint64_t *pos_of_site);

/* ---- the exchange steps of the sharded path: RCCL over xGMI, one process per GPU ------------------------
 * The reference fans out one process per sample (run.py:704-718, `run_array` with `max_processes`) over a shared file system
 * and has no exchange step; sharded over GPUs the hot path has three: C1, the all-gather of the per-rank SNP site keys
 * (variable length: snpgpu_allgatherv); C2, the all-gather of the per-rank rows of the packed consensus matrix
 * (snpgpu_allgather, or snpgpu_allgatherv when the last rank holds fewer rows); the row-band exchange of the 128 x 128
 * distance tiles (snpgpu_tiles_gather_dev -> snpgpu_alltoallv -> snpgpu_tiles_scatter_dev).  librccl.so is loaded on first
 * use (snpgpu_comm_available() == 0: not found; single-GPU work is not affected).  Rank 0 makes a 128-byte id and hands it
 * to the other ranks by any means the host program has; every rank then calls snpgpu_comm_init on its own context (its own
 * device).  The collectives are ENQUEUED on the context's stream, like kernels: they return at once, results are valid when
 * the stream has passed them (snpgpu_ctx_sync, or snpgpu_stream_wait with a time limit: a rank that never arrives shows as
 * SNPGPU_E_TIMEOUT instead of a process that hangs).  All ranks must make the same calls in the same order. */
#define SNPGPU_COMM_ID_BYTES 128
int  snpgpu_comm_available(void);
int  snpgpu_comm_version(int *out_version);                    /* ncclGetVersion of the library that was loaded */
int  snpgpu_comm_unique_id(void *out_id);                      /* SNPGPU_COMM_ID_BYTES bytes; rank 0 */
int  snpgpu_comm_init(snpgpu_ctx *ctx, int rank, int nranks, const void *unique_id);
void snpgpu_comm_destroy(snpgpu_ctx *ctx);                     /* (also done by snpgpu_ctx_destroy) */
void snpgpu_comm_abort(snpgpu_ctx *ctx);                       /* without waiting for the stream: cancels what never completed (ncclCommAbort) */
/* this rank, the number of ranks, and what ncclCommCount says (0 without a communicator) */
int  snpgpu_comm_info(const snpgpu_ctx *ctx, int *out_rank, int *out_nranks, int *out_count_from_rccl);
/* block r of d_recv (bytes_per_rank bytes) comes from rank r's d_send */
int  snpgpu_allgather(snpgpu_ctx *ctx, const void *d_send, void *d_recv, size_t bytes_per_rank);
/* rank r contributes bytes[r] bytes, which land at d_recv + offsets[r] on every rank; bytes / offsets: HOST arrays of nranks
 * entries, the same on every rank (sizes are exchanged first, e.g. with snpgpu_allgather of one word) */
int  snpgpu_allgatherv(snpgpu_ctx *ctx, const void *d_send, void *d_recv, const uint64_t *bytes, const uint64_t *offsets);
/* send_bytes[p] bytes of d_send (blocks packed in rank order) go to rank p; recv_bytes[p] bytes from rank p arrive in d_recv
 * (blocks packed in rank order); HOST arrays */
int  snpgpu_alltoallv(snpgpu_ctx *ctx, const void *d_send, const uint64_t *send_bytes, void *d_recv, const uint64_t *recv_bytes);
int  snpgpu_stream_wait(snpgpu_ctx *ctx, uint32_t timeout_ms);
/* 128 x 128 tiles of an n_padded x n_padded int32 matrix (n_padded a multiple of 128) to and from a packed list: tile t is the
 * block at tile row d_tile_rows[t], tile column d_tile_cols[t]; d_out / d_tiles hold 128 * 128 values per tile */
int  snpgpu_tiles_gather_dev(snpgpu_ctx *ctx, const int32_t *d_matrix, uint32_t n_padded, const uint32_t *d_tile_rows,
                             const uint32_t *d_tile_cols, uint32_t n_tiles, int32_t *d_out);
int  snpgpu_tiles_scatter_dev(snpgpu_ctx *ctx, const int32_t *d_tiles, const uint32_t *d_tile_rows, const uint32_t *d_tile_cols,
                              uint32_t n_tiles, int32_t *d_matrix, uint32_t n_padded);
/* What the one-job pipeline asks about a group of samples after scan + call, per sample s -> d_out[s][3] (int64): [0] 1 when a
 * position the sample is asked about is malformed (d_wanted[n_sites]: 1 = every sample is asked about it; plus the sample's
 * own stretch d_excl_slots[d_excl_off[s] .. d_excl_off[s + 1]), both nullable), judged by the records' status bytes when
 * d_counts is given, else by bit 7 of the filter bytes; [1] positions of the set that have a pileup line (d_line_off != 0);
 * [2] positions with a record in the context's spill (d_counts only).  Inputs [n_samples][n_sites]. */
int  snpgpu_group_check_dev(snpgpu_ctx *ctx, const uint8_t *d_filters, const snpgpu_site_counts *d_counts, const uint64_t *d_line_off,
                            const uint8_t *d_wanted, const uint32_t *d_excl_off, const uint32_t *d_excl_slots,
                            uint32_t n_samples, uint32_t n_sites, int64_t *d_out);

/* ---- filter_regions: find_dense_regions (filter_regions.py:17-71) + utils.merge_regions
 *      (utils.py:1267-1282) + utils.in_region (utils.py:1314-1318); merge_sites (merge_sites.py:91-117) ---------
 * Hand-written sort / scan kernels (csrc/prims.h); each step comes as a host-pointer form (synchronous, one
 * synchronisation at its end) and a `_dev` form (device pointers, asynchronous on the context's stream, counts left in
 * device memory: d_out_n[0] = number of outputs, d_out_n[1] = error bits — 1: position outside [0, 2^40),
 * 2: interval with start > end).  Output capacities are stated with each function.
 *
 * dense windows: positions are grouped in segments (one per (sample, contig)); seg_off[n_segs+1]; the positions of a
 * segment may come in any order (they are sorted on the device, filter_regions.py:425).  For every rule r the candidate
 * window (p[i], p[i+max_snps[r]]) is emitted when p[i] + window[r] - 1 >= p[i+max_snps[r]].  out_start/out_end receive the
 * candidates (capacity n_pos * n_rules), out_seg their segment; order: by segment, position, rule.  At most 64 rules. */
int  snpgpu_dense_windows(snpgpu_ctx *ctx, const int64_t *positions, const uint32_t *seg_off, uint32_t n_segs,
                          const int32_t *max_snps, const int32_t *window, uint32_t n_rules,
                          int64_t *out_start, int64_t *out_end, uint32_t *out_seg, uint32_t *out_n);
int  snpgpu_dense_windows_dev(snpgpu_ctx *ctx, const int64_t *d_positions, const uint32_t *d_seg_off, uint32_t n_segs,
                              uint32_t n_pos, const int32_t *max_snps /* host */, const int32_t *window /* host */,
                              uint32_t n_rules, int64_t *d_out_start, int64_t *d_out_end, uint32_t *d_out_seg,
                              uint32_t *d_out_n /* 2 words */);
/* Merge intervals per group (intervals in any order, start <= end): sort by (group,start,end), running max of end, join
 * when start <= last_end + 1.  Output: merged regions ascending by (group, start); capacity n. */
int  snpgpu_merge_regions(snpgpu_ctx *ctx, const uint32_t *group, const int64_t *start, const int64_t *end,
                          uint32_t n, uint32_t *out_group, int64_t *out_start, int64_t *out_end, uint32_t *out_n);
int  snpgpu_merge_regions_dev(snpgpu_ctx *ctx, const uint32_t *d_group, const int64_t *d_start, const int64_t *d_end,
                              uint32_t n, uint32_t *d_out_group, int64_t *d_out_start, int64_t *d_out_end,
                              uint32_t *d_out_n /* 2 words */);
/* in_region for many positions: regions per group must be merged (disjoint, sorted); reg_off[n_groups+1].
 * out_flag[i] = 1 when positions[i] lies in a region of pos_group[i] (inclusive ends). */
int  snpgpu_in_regions(snpgpu_ctx *ctx, const uint32_t *pos_group, const int64_t *positions, uint32_t n_pos,
                       const uint32_t *reg_off, const int64_t *reg_start, const int64_t *reg_end,
                       uint32_t n_groups, uint8_t *out_flag);
int  snpgpu_in_regions_dev(snpgpu_ctx *ctx, const uint32_t *d_pos_group, const int64_t *d_positions, uint32_t n_pos,
                           const uint32_t *d_reg_off, const int64_t *d_reg_start, const int64_t *d_reg_end,
                           uint32_t n_groups, uint8_t *d_out_flag);

/* merge_sites: union of (CHROM,POS) over samples (merge_sites.py:91-117).
 * keys[i] = (contig_index << 32) | pos, sample_of_key[i] = sample index in sorted-dir order; records in any order.
 * Outputs: unique keys ascending, CSR offsets (n_unique+1) and the carrier sample indices in ascending
 * order per key, duplicates of (key, sample) collapsed (the reference builds a set per sample).
 * Capacities: out_unique[n], out_off[n+1], out_carrier[n].  _dev: d_out_n[0] = unique keys, d_out_n[1] = carriers. */
int  snpgpu_merge_sites(snpgpu_ctx *ctx, const uint64_t *keys, const uint32_t *sample_of_key, size_t n,
                        uint64_t *out_unique, uint32_t *out_off, uint32_t *out_carrier,
                        uint32_t *out_n_unique, uint32_t *out_n_carrier);
int  snpgpu_merge_sites_dev(snpgpu_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_sample_of_key, uint32_t n,
                            uint64_t *d_out_unique, uint32_t *d_out_off, uint32_t *d_out_carrier,
                            uint32_t *d_out_n /* 2 words */);

/* ---- synthetic pileups for bench/tests, generated on the device --------------------
 * Fills d_out with the text of one sample's pileup over a single contig and returns its length in *out_nbytes
 * (synchronous; d_out capacity in bytes; d_out == NULL only queries the length).  d_site_alt[genome_len+1]: 0 or the ALT base at each 1-based position. */
typedef struct snpgpu_synth_params {
    uint64_t seed;
    uint32_t sample;
    uint32_t genome_len;
    float    mean_depth;
    float    carrier_p_same_clade;
    float    carrier_p_other_clade;
    uint32_t n_clades;
    char     contig[32];
} snpgpu_synth_params;
int  snpgpu_synth_reference_dev(snpgpu_ctx *ctx, uint64_t seed, uint32_t genome_len, uint8_t *d_ref /* genome_len+1 */);
int  snpgpu_synth_pileup_dev(snpgpu_ctx *ctx, const snpgpu_synth_params *p, const uint8_t *d_ref,
                             const uint8_t *d_site_alt, uint8_t *d_out, size_t capacity, size_t *out_nbytes);

/* ---- BGZF-compressed pileups (`samtools mpileup | bgzip`): index on the host, inflate on the device ---------------
 * (Additive in ABI 7.)  A BGZF file is a series of gzip members ("blocks") of at most 64 KiB of text each, every one with
 * its compressed size in an extra subfield `BC`, so the blocks can be found without decoding and inflated independently.
 * The index walks the headers; the inflate kernel takes one block per wave, decodes it into a 64 KiB window in LDS,
 * checks its CRC32 there and writes the text at the block's plain offset.  A bad block is a status, never a fault. */
#define SNPGPU_BGZF_E_NOT_GZIP   -101  /* no gzip magic at the start: the caller treats the file as plain text */
#define SNPGPU_BGZF_E_NOT_BGZF   -102  /* gzip, but no BC subfield: unsupported ("recompress with bgzip") */
#define SNPGPU_BGZF_E_TRUNCATED  -103  /* a block runs past the end of the data */
#define SNPGPU_BGZF_E_ISIZE      -104  /* a block promises more than 65 536 bytes of text */
#define SNPGPU_BGZF_E_MAGIC      -105  /* bad magic or header in mid-file */
/* status of one block after inflate */
#define SNPGPU_BGZF_ST_OK           0
#define SNPGPU_BGZF_ST_BTYPE        1  /* reserved deflate block type */
#define SNPGPU_BGZF_ST_STORED_LEN   2  /* stored block: LEN and NLEN disagree */
#define SNPGPU_BGZF_ST_CODE_SET     3  /* over-subscribed or incomplete code lengths, bad repeat, no end-of-block code */
#define SNPGPU_BGZF_ST_SYMBOL       4  /* bits that are no code of the set, or a reserved length / distance symbol */
#define SNPGPU_BGZF_ST_DISTANCE     5  /* a match reaches before the block's own first byte */
#define SNPGPU_BGZF_ST_INPUT_END    6  /* the bit stream ends before its end-of-block code */
#define SNPGPU_BGZF_ST_OUTPUT_OVER  7  /* more text than ISIZE */
#define SNPGPU_BGZF_ST_OUTPUT_SHORT 8  /* less text than ISIZE */
#define SNPGPU_BGZF_ST_CRC          9  /* CRC32 of the text differs from the footer's */
typedef struct snpgpu_bgzf_block {
    uint64_t coff;       /* offset of the block (its gzip header) in the compressed data */
    uint64_t poff;       /* offset of its text in the plain data */
    uint32_t csize;      /* BSIZE + 1: the whole block */
    uint32_t isize;      /* bytes of text, at most 65 536 */
    uint32_t crc;        /* CRC32 of the text */
    uint32_t data_off;   /* the deflate stream lies at [coff + data_off, coff + csize - 8) */
} snpgpu_bgzf_block;
typedef struct snpgpu_bgzf_info {
    uint64_t n_blocks, plain_bytes, compressed_bytes;
    uint64_t bad_block;      /* first block in error (index or inflate), UINT64_MAX: none */
    uint64_t bad_offset;     /* its compressed offset */
    int32_t  index_rc;       /* what the index said: 0 or SNPGPU_BGZF_E_* */
    uint32_t bad_status;     /* SNPGPU_BGZF_ST_* of bad_block after inflate */
    uint32_t n_bad;          /* blocks whose status is not OK */
    uint32_t has_eof_marker; /* the file ends in the 28-byte empty block (its absence is accepted, as htslib accepts it) */
    uint64_t reserved[2];
} snpgpu_bgzf_info;
/* 1: BGZF, 0: not gzip (plain text), SNPGPU_E_IO: cannot be read, SNPGPU_BGZF_E_NOT_BGZF / _TRUNCATED: gzip that is no BGZF.
 * Reads the first block header only. */
int  snpgpu_bgzf_probe(const char *path);
const char *snpgpu_bgzf_strerror(int code);          /* the SNPGPU_BGZF_E_* codes in words */
const char *snpgpu_bgzf_status_name(uint32_t status);
/* The block table of data[0, nbytes) (host memory, no context).  *out_n: the number of blocks; at most `capacity` of them are
 * written (capacity 0 only counts).  Returns 0 or the SNPGPU_BGZF_E_* of the first bad header (info->bad_offset says where;
 * the blocks before it are valid and counted).  info is nullable. */
int  snpgpu_bgzf_index(const uint8_t *data, uint64_t nbytes, snpgpu_bgzf_block *out_blocks, uint64_t capacity, uint64_t *out_n,
                       snpgpu_bgzf_info *info);
/* Device to device: the blocks h_blocks[0, n_blocks) (a HOST table) of d_compressed[0, compressed_bytes) inflated to
 * d_out[poff, poff + isize).  Before any launch the table is checked on the host: a block that leaves the compressed data, or
 * whose text would pass out_capacity, is SNPGPU_E_ARG.  h_block_status (nullable) receives one SNPGPU_BGZF_ST_* per block; a bad
 * block leaves its text unwritten and every other block untouched.  Synchronous.  Returns 0 also when blocks are bad: see
 * info->n_bad / bad_block / bad_status (info nullable). */
int  snpgpu_bgzf_inflate_dev(snpgpu_ctx *ctx, const void *d_compressed, uint64_t compressed_bytes, const snpgpu_bgzf_block *h_blocks,
                             uint64_t n_blocks, void *d_out, uint64_t out_capacity, uint32_t *h_block_status, snpgpu_bgzf_info *info);
/* One block on the host with the decoder the kernel runs: block[0, b->csize) -> out[0, b->isize).  Returns its status. */
uint32_t snpgpu_bgzf_inflate_block_host(const uint8_t *block, const snpgpu_bgzf_block *b, uint8_t *out);
/* Host only: the plain bytes [plain_offset, plain_offset + nbytes) of a BGZF file (fewer at the end of the text: *out_n),
 * from the index and the host inflater.  SNPGPU_E_IO, SNPGPU_E_PILEUP (bad block) or a SNPGPU_BGZF_E_* code on failure. */
int  snpgpu_bgzf_read_range(const char *path, uint64_t plain_offset, uint64_t nbytes, uint8_t *out, uint64_t *out_n);
/* snpgpu_call_consensus_files for BGZF files: arguments and outputs as there, plus out_info [n_files] (nullable).  Each
 * file's compressed bytes go through the reader threads and the pinned ring to the device, are inflated there into a text
 * buffer sized from the index, and scanned and called like a resident pileup.  out_line_off is 1 + the offset in the PLAIN
 * text.  out_rc: SNPGPU_E_IO for a file that cannot be read or is truncated, SNPGPU_E_UNSUPPORTED for one that is no BGZF,
 * SNPGPU_E_PILEUP for a bad block (CRC, ISIZE, deflate stream) — the block and the cause are in out_info and in
 * snpgpu_last_error; the rows of such a file are '-' / 0 / no line.  SNPGPU_E_NOMEM when the text buffer cannot be had.
 * Limitation: one file at a time.  There is one compressed slot and one text slot; the read, copy and inflate of file k+1 do
 * NOT overlap the scan and call of file k (each file is loaded and inflated synchronously, then scanned as device text).
 * stats: bytes (PLAIN text that was scanned), n_chunks (files that were inflated), seconds, seconds_waiting_for_device and
 * seconds_enqueueing are filled; n_readers, n_staging, chunk_bytes and the reader seconds stay 0. */
int  snpgpu_call_consensus_bgzf_files(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const char *const *paths, uint32_t n_files,
                                      const snpgpu_caller_params *params, const uint32_t *excl_off, const uint32_t *excl_slots,
                                      uint8_t *out_base, uint8_t *out_filters,
                                      snpgpu_site_counts *out_counts, uint64_t *out_line_off, uint64_t *out_status,
                                      int32_t *out_rc, const snpgpu_stream_opts *opts, snpgpu_stream_stats *stats,
                                      snpgpu_bgzf_info *out_info);

#ifdef __cplusplus
}
#endif
#endif /* SNPGPU_H */
