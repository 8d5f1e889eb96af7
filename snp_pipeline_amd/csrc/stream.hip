// Everything this project moves from disk to the device: pileup files (or host buffers) and VCF files, streamed through
// pinned memory without ever waiting for a whole file to be read.
//
// Replaces the way the reference feeds pileup.Reader (snppipeline/pileup.py:408-429: a text-mode line iterator over the
// open file, driven from call_consensus.py:161) and the one-process-per-sample job array around it (run.py:704-718).
// A pileup is 0.4 GB of text per 5 Mbp x 30x sample: the 10 000-sample target is 4 TB that can only pass through HBM,
// so the rate that matters end to end is the host link's, and the job of this file is to keep that link busy:
//
//   reader threads   pread() the files (page cache) piece by piece into a ring of PINNED staging buffers — a kernel-side
//                    memcpy of ~5 GB/s per thread, hence several threads.  They never call HIP.
//   issuing thread   waits for piece j, retires finished copies by polling their events (a staging buffer is refilled only
//                    after the copy out of it has completed), copies the piece on one of two copy streams and records the
//                    buffer's event.  Nobody waits after an abort.
// That mechanism is Ring; what a consumer does between Ring::wait(j) and the recording of the copy event is its own.
//
// In file order:
//   pool             the pinned staging buffers, copy streams and events, device slots and result blocks a context keeps
//   Opener           opens the files of a batch a few ahead of the readers
//   Ring             the in-order staging ring and its readers (read_piece, start_readers / stop_readers)
//   run_stream       call_consensus over files or host buffers, in chunks of whole 4 KiB scan tiles.  On top of the ring:
//                    times the wait; a read error marks the file SNPGPU_E_IO; the compute stream waits on the copy event
//                    and scans the tiles that are now complete (tile + 128-byte halo inside the landed bytes; scan.hip:
//                    snpgpu_scan_range).  Lines the fast parser leaves to the exact parser are queued with their file
//                    offsets and finished when the file is complete, as is the call step (snpgpu_enqueue_call), which
//                    reads the lines the scan selected straight from the file's device buffer ("slot"); results come
//                    back through pinned blocks.  Files alternate between n_slots slots, so file k+1 streams in while
//                    file k's tail runs; the compute stream is in order, so all device scratch is shared between files.
//   one-file loads   load_raw (and load_bgzf / load_file on it).  No opener thread; a read error fails the whole call; the
//                    compute stream waits on nothing, both copy streams are synchronised at the end.
//   all lines        --vcfAllPos: a record, or a VCF row, for every line of one loaded file
//   site calling     varscan_resident(_batch) over text in device memory; varscan_stream over files, and the resident
//                    store behind it.  Pass A copies the pieces of resident files in ANY order (its own retire loop);
//                    pass B is the ring over jobs [JA, J), with opportunistic() before each wait.
//   VCF streams      vcf_stream: pieces into a few device buffers, counted or parsed by a launch each.  The host may
//                    append '\n' to the staged piece before the copy, and the copy also waits on ev_counted[b].
//   merge_vcfs       the multi-sample VCF from the parsed pieces (vcf_merge.hip)
#include <errno.h>
#include <fcntl.h>
#include <sched.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include <algorithm>

#include <unordered_map>

#include "internal.h"

namespace {

inline size_t up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Source {
    const char *path = nullptr;     // a file ...
    const uint8_t *mem = nullptr;   // ... or host memory
    const uint8_t *dev = nullptr;   // ... or text that is already in device memory (an inflated BGZF file): nothing to read or copy
    uint64_t size = 0;
    int fd = -1;
    int rc = SNPGPU_OK;
};

struct Job {
    uint32_t file;
    uint64_t off, len;
    bool first, last;
    uint32_t chunk;                 // index of the chunk inside its file
};

// In a function with `int rc` and a `done:` label behind which everything is undone (#undef'd where the last namespace ends).
#define STREAM_TRY(expr)                                                                                            \
    do {                                                                                                            \
        hipError_t e_ = (expr);                                                                                     \
        if (e_ != hipSuccess) { rc = snpgpu_set_error(ctx, SNPGPU_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); goto done; } \
    } while (0)

// The size of a file source.  What is no regular file is an I/O error of that file, with nothing to read.
void size_source(Source &s) {
    struct stat stt;
    if (!s.path || stat(s.path, &stt) != 0 || !S_ISREG(stt.st_mode)) {
        s.rc = SNPGPU_E_IO;
        s.size = 0;
    } else {
        s.size = (uint64_t)stt.st_size;
    }
}

// Readers and staging buffers for J jobs: no more readers than jobs, extra_staging buffers beyond one per reader, at least one.
void ring_sizes(uint64_t J, uint32_t n_readers_wanted, uint32_t extra_staging, uint32_t *n_readers, uint32_t *n_staging) {
    *n_readers = n_readers_wanted > J ? (uint32_t)J : n_readers_wanted;
    *n_staging = *n_readers + extra_staging;
    if (*n_staging > J) *n_staging = (uint32_t)J;
    if (*n_staging < 1) *n_staging = 1;
}

// The first pieces of a load are small — 1, 1, 2, 4, 8 MiB, then `chunk` — so that the first copy starts after ~1 MiB has been
// read instead of after a whole chunk (all readers start at once and each takes a few milliseconds per 16 MiB).
inline uint64_t ramp_piece(uint64_t c, uint64_t chunk) { return c < 2 ? (uint64_t)1 << 20 : (c < 5 ? (uint64_t)1 << (18 + c) : chunk); }

// The files of a batch are opened by a thread of their own, a few files ahead of the readers, and each is closed by the reader
// that reads its last piece: at most OPEN_WINDOW of them are open at a time.  Opening all of them up front is what costs: a
// process whose descriptor table has to grow beyond its current size waits for an RCU grace period per doubling while the
// table is shared between threads (expand_fdtable), and so does every other thread that needs a descriptor meanwhile — 0.3 s
// for the 125 files of a job on the 256-CPU box, and the pinning of the staging memory stood still with it
// (tools/pipeline_time.py --probe-open, tools/probe/open_stall_probe.py).  Sizes come from stat(); a file that cannot be opened, or
// has become smaller than stat() said, is an I/O error of that file (its pieces are read as blank lines).
struct Opener {
    static constexpr uint32_t OPEN_WINDOW = 16;
    std::vector<Source> *src = nullptr;
    std::unique_ptr<std::atomic<uint8_t>[]> opened;
    std::unique_ptr<std::atomic<uint32_t>[]> reads_left;        // pieces of the file not read yet
    std::atomic<uint32_t> n_closed{0};
    std::atomic<bool> stop{false};
    std::thread th;

    void open_one(Source &s) const {
        if (s.rc != SNPGPU_OK || s.size == 0 || !s.path) return;
        s.fd = open(s.path, O_RDONLY | O_CLOEXEC);
        struct stat stt;
        if (s.fd < 0 || fstat(s.fd, &stt) != 0 || !S_ISREG(stt.st_mode) || (uint64_t)stt.st_size < s.size) {
            if (s.fd >= 0) { close(s.fd); s.fd = -1; }
            s.rc = SNPGPU_E_IO;
            return;
        }
        (void)posix_fadvise(s.fd, 0, 0, POSIX_FADV_SEQUENTIAL);
    }
    void run() {
        for (size_t f = 0; f < src->size(); ++f) {
            while (!stop.load(std::memory_order_relaxed) && f >= (size_t)n_closed.load(std::memory_order_acquire) + OPEN_WINDOW)
                std::this_thread::sleep_for(std::chrono::microseconds(50));
            if (!stop.load(std::memory_order_relaxed)) open_one((*src)[f]);
            opened[f].store(1, std::memory_order_release);       // (after a cancel: nobody reads any more, nobody may wait either)
        }
    }
    // pieces[f]: the number of jobs of file f (each of them ends in one done_reading(f))
    void start(std::vector<Source> *sources, const std::vector<uint32_t> &pieces) {
        src = sources;
        const size_t n = sources->size() ? sources->size() : 1;
        opened.reset(new std::atomic<uint8_t>[n]);
        reads_left.reset(new std::atomic<uint32_t>[n]);
        for (size_t f = 0; f < sources->size(); ++f) {
            opened[f].store(0, std::memory_order_relaxed);
            reads_left[f].store(pieces[f], std::memory_order_relaxed);
        }
        try { th = std::thread(&Opener::run, this); } catch (const std::exception &) { stop.store(true); run(); stop.store(false); open_all_now(); }
    }
    void open_all_now() { for (auto &s : *src) open_one(s); }   // no thread to be had: everything up front after all
    void wait(uint32_t f) const {
        while (!opened[f].load(std::memory_order_acquire)) std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    void done_reading(uint32_t f) {                             // by the reader that has just read (or skipped) a piece of file f
        if (reads_left[f].fetch_sub(1, std::memory_order_acq_rel) != 1) return;
        Source &s = (*src)[f];
        if (s.fd >= 0 && s.path) { close(s.fd); s.fd = -1; }
        n_closed.fetch_add(1, std::memory_order_release);
    }
    void cancel() { stop.store(true); }                         // before the readers are told to give up: none of them may wait for a file
    void finish() {
        stop.store(true);
        if (th.joinable()) th.join();
    }
};

}  // namespace

// Persistent per-context resources of the streaming path (pinned memory is expensive to allocate: keep it).
struct snpgpu_stream_pool {
    hipStream_t copy_stream = nullptr;      // chunks alternate between two copy streams: the set-up of one copy hides
    hipStream_t copy_stream2 = nullptr;     // behind the transfer of the other
    cpu_set_t near_cpus;                    // CPUs of the NUMA node the device hangs off (reader threads run there)
    bool have_near_cpus = false;
    size_t chunk_bytes = 0;
    std::vector<void *> staging;            // pinned, chunk_bytes each
    std::vector<hipEvent_t> ev_copy;        // the H2D copy out of staging[i] has completed
    std::vector<void *> slot;               // device file buffers
    size_t slot_bytes = 0;
    std::vector<hipEvent_t> ev_done;        // the results of the file in slot i are in its pinned result block
    std::vector<void *> result;             // pinned result blocks, one per slot
    size_t result_bytes = 0;
    std::vector<void *> table_host;         // pinned mirrors of the per-chunk sample tables, one per slot
    size_t table_bytes = 0;
};

static void pool_free_host(std::vector<void *> &v) {
    for (void *p : v) if (p) (void)hipHostFree(p);
    v.clear();
}

void snpgpu_stream_pool_destroy(snpgpu_ctx *ctx) {
    snpgpu_stream_pool *p = ctx->pool;
    if (!p) return;
    pool_free_host(p->staging);
    pool_free_host(p->result);
    pool_free_host(p->table_host);
    for (void *d : p->slot) if (d) (void)hipFree(d);
    for (auto e : p->ev_copy) (void)hipEventDestroy(e);
    for (auto e : p->ev_done) (void)hipEventDestroy(e);
    if (p->copy_stream) (void)hipStreamDestroy(p->copy_stream);
    if (p->copy_stream2) (void)hipStreamDestroy(p->copy_stream2);
    delete p;
    ctx->pool = nullptr;
}

namespace {

// n_slots device file buffers of slot_bytes; n_blocks (>= n_slots) pinned result blocks, table mirrors and done-events — files
// that go to resident memory (snpgpu_pileups) need the blocks but no slot
int pool_ensure(snpgpu_ctx *ctx, size_t chunk_bytes, uint32_t n_staging, uint32_t n_slots, size_t slot_bytes, size_t result_bytes,
                size_t table_bytes, uint32_t n_blocks = 0) {
    if (n_blocks < n_slots) n_blocks = n_slots;
    if (!ctx->pool) ctx->pool = new snpgpu_stream_pool();
    snpgpu_stream_pool *p = ctx->pool;
    if (!p->copy_stream) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking));
        HIP_TRY(ctx, hipStreamCreateWithFlags(&p->copy_stream2, hipStreamNonBlocking));
        // the CPUs next to the device: /sys/bus/pci/devices/<bdf>/local_cpulist (best effort)
        char bdf[64] = {0};
        if (hipDeviceGetPCIBusId(bdf, sizeof bdf, ctx->device) == hipSuccess) {
            for (char *c = bdf; *c; ++c) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
            char path[160];
            snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/local_cpulist", bdf);
            if (FILE *fp = fopen(path, "r")) {
                char line[1024] = {0};
                if (fgets(line, sizeof line, fp)) {
                    CPU_ZERO(&p->near_cpus);
                    int n_set = 0;
                    for (char *tok = strtok(line, ",\n"); tok; tok = strtok(nullptr, ",\n")) {
                        int a = 0, b = 0;
                        const int k = sscanf(tok, "%d-%d", &a, &b);
                        if (k == 1) b = a;
                        if (k >= 1) for (int c = a; c <= b && c < CPU_SETSIZE; ++c) { CPU_SET(c, &p->near_cpus); ++n_set; }
                    }
                    p->have_near_cpus = n_set > 0;
                }
                fclose(fp);
            }
        }
    }
    if (p->chunk_bytes != chunk_bytes) {
        pool_free_host(p->staging);
        p->chunk_bytes = chunk_bytes;
    }
    while (p->staging.size() < n_staging) {
        void *h = nullptr;
        hipError_t e = hipHostMalloc(&h, chunk_bytes, hipHostMallocDefault);
        if (e != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipHostMalloc(%zu) failed: %s", chunk_bytes, hipGetErrorString(e));
        p->staging.push_back(h);
    }
    while (p->ev_copy.size() < p->staging.size()) {
        hipEvent_t ev = nullptr;
        HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        p->ev_copy.push_back(ev);
    }
    if (p->slot_bytes < slot_bytes || p->slot.size() < n_slots) {
        for (void *d : p->slot) if (d) (void)hipFree(d);
        p->slot.clear();
        const size_t want = p->slot_bytes > slot_bytes ? p->slot_bytes : slot_bytes;
        for (uint32_t i = 0; i < n_slots; ++i) {
            void *d = nullptr;
            hipError_t e = hipMalloc(&d, want);
            if (e != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc(%zu) for a pileup slot failed: %s", want, hipGetErrorString(e));
            p->slot.push_back(d);
        }
        p->slot_bytes = want;
    }
    if (n_blocks < p->slot.size()) n_blocks = (uint32_t)p->slot.size();
    while (p->ev_done.size() < n_blocks) {
        hipEvent_t ev = nullptr;
        HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        p->ev_done.push_back(ev);
    }
    // n pinned blocks of at least bytes_want each: all of them anew when there are too few or they are too small, never smaller
    auto grow_pinned = [&](std::vector<void *> &vec, size_t n, size_t &bytes_have, size_t bytes_want) -> int {
        if (bytes_have >= bytes_want && vec.size() >= n) return SNPGPU_OK;
        pool_free_host(vec);
        if (bytes_want < bytes_have) bytes_want = bytes_have;
        for (size_t i = 0; i < n; ++i) {
            void *h = nullptr;
            hipError_t e = hipHostMalloc(&h, bytes_want, hipHostMallocDefault);
            if (e != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipHostMalloc(%zu) failed: %s", bytes_want, hipGetErrorString(e));
            vec.push_back(h);
        }
        bytes_have = bytes_want;
        return SNPGPU_OK;
    };
    if (int rc = grow_pinned(p->result, n_blocks, p->result_bytes, result_bytes)) return rc;
    return grow_pinned(p->table_host, n_blocks, p->table_bytes, table_bytes);
}

struct Outputs {
    uint8_t *base, *filters;
    snpgpu_site_counts *counts;     // nullable
    uint64_t *line_off;             // nullable
    uint64_t *status;
    int32_t *rc;                    // nullable
    bool on_device = false;         // base / filters / counts / line_off are DEVICE arrays: the kernels of file f write row f
                                    // themselves, only the status words pass through the pinned result block
};

// One piece of a source into staging memory.  Returns the errno of a failed read (0: fine); whatever could not be read is
// filled with newlines, so that the piece is blank lines to the kernels.
int read_piece(Source &s, const Job &jb, uint8_t *dst) {
    if (s.mem) {
        memcpy(dst, s.mem + jb.off, jb.len);
        return 0;
    }
    int err = 0;
    uint64_t got = 0;
    while (s.fd >= 0 && got < jb.len) {                     // (no descriptor: could not be opened, its result is void and rc says so)
        ssize_t r = pread(s.fd, dst + got, jb.len - got, (off_t)(jb.off + got));
        if (r < 0) { if (errno == EINTR) continue; err = errno ? errno : EIO; break; }
        if (r == 0) { err = EIO; break; }                    // the file shrank under us
        got += (uint64_t)r;
    }
    if (got < jb.len) memset(dst + got, '\n', jb.len - got);
    return err;
}

// The reader threads of a Shared or an AnyOrder (below) take jobs [sh.next, n_jobs) off a counter.  stop_readers ends them:
// after a failure they are told to give up — the opener first, so that none of them waits for a file, then `abort` for those that
// wait on cv — otherwise they run out of jobs by themselves.  Safe to call again.
template <class S>
void stop_readers(S &sh, std::condition_variable &cv, uint64_t n_jobs, bool failed) {
    if (sh.readers.empty()) return;
    if (failed && sh.opener) sh.opener->cancel();
    {
        std::lock_guard<std::mutex> lk(sh.mu);
        if (failed) { sh.abort = true; sh.next.store(n_jobs); }
    }
    cv.notify_all();
    for (auto &t : sh.readers) t.join();
    sh.readers.clear();
}

// size(): sizes what the readers share; then n threads that run main_fn(ctx, &sh, jobs, src).  No memory for the one or no thread for
// the other is an error code, never an exception through the C ABI, and the threads that did start are stopped again.
template <class S, class Size>
int start_readers(snpgpu_ctx *ctx, S &sh, std::condition_variable &cv, uint64_t n_jobs, uint32_t n, Size size,
                  void (*main_fn)(snpgpu_ctx *, S *, const std::vector<Job> *, std::vector<Source> *), const std::vector<Job> *jobs,
                  std::vector<Source> *src) {
    try {
        size();
        for (uint32_t i = 0; i < n; ++i) sh.readers.emplace_back(main_fn, ctx, &sh, jobs, src);
    } catch (const std::exception &e) {                     // nothing has been enqueued yet
        stop_readers(sh, cv, n_jobs, true);
        return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "cannot start the reader threads: %s", e.what());
    }
    return SNPGPU_OK;
}

// What the readers and the issuing thread of the in-order ring share.
struct Shared {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<uint8_t> filled;    // [job - base] the job has been read into its staging buffer
    std::vector<int> job_err;       // [job - base] errno of a failed read (0: fine)
    int64_t freed = 0;              // places of the ring whose H2D copy has completed: their staging buffers can be refilled
    uint64_t R = 1;                 // staging buffers in the ring
    std::atomic<uint64_t> ns_reading{0}, ns_waiting{0};   // summed over the readers
    bool abort = false;
    std::atomic<uint64_t> next{0};
    uint64_t base = 0, end = 0;     // the ring serves jobs [base, end): job j has place j - base and uses staging[(j - base) % R]
    Opener *opener = nullptr;       // (optional) the files are opened by another thread and closed by the last reader
    std::vector<std::thread> readers;
};

void reader_main(snpgpu_ctx *ctx, Shared *sh, const std::vector<Job> *jobs, std::vector<Source> *src) {
    snpgpu_stream_pool *p = ctx->pool;
    if (p->have_near_cpus) (void)sched_setaffinity(0, sizeof p->near_cpus, &p->near_cpus);   // this thread only; best effort
    const uint64_t R = sh->R;
    for (;;) {
        const uint64_t j = sh->next.fetch_add(1);
        if (j >= sh->end) return;
        const Job &jb = (*jobs)[j];
        const double t_w = now_s();
        const uint64_t k = j - sh->base;                    // place in the ring
        if (k >= R) {                                       // staging[k % R] is free once the job R places before has been copied out of it
            std::unique_lock<std::mutex> lk(sh->mu);         // (the issuing thread watches the copy events: readers never call HIP)
            sh->cv.wait(lk, [&] { return sh->abort || sh->freed > (int64_t)(k - R); });
            if (sh->abort) return;
        }
        const double t_r = now_s();
        if (sh->opener) sh->opener->wait(jb.file);
        const int err = read_piece((*src)[jb.file], jb, (uint8_t *)p->staging[k % R]);
        if (sh->opener) sh->opener->done_reading(jb.file);
        sh->ns_waiting.fetch_add((uint64_t)((t_r - t_w) * 1e9));
        sh->ns_reading.fetch_add((uint64_t)((now_s() - t_r) * 1e9));
        {
            std::lock_guard<std::mutex> lk(sh->mu);
            sh->filled[k] = 1;
            sh->job_err[k] = err;
        }
        sh->cv.notify_all();
    }
}

// The in-order staging ring: reader threads fill staging[(j - base) % R] with job j; the issuing thread — the only one that calls
// HIP — takes the jobs in order: wait(j), then the copy out of staging(j) on copy_stream(j), then copy_event(j) recorded behind
// it.  A staging buffer goes back to the readers only when the copy out of it has completed, which wait() learns by polling the
// events in order.
struct Ring : Shared {
    snpgpu_stream_pool *p = nullptr;
    int64_t copies_done = 0;        // the copies of places [0, copies_done) have completed

    // Readers for jobs [first_job, first_job + n_jobs) over the first R staging buffers of the pool.  opener: nullptr when the
    // sources are open already.  On failure nothing is left running.
    int start(snpgpu_ctx *ctx, const std::vector<Job> *jobs, std::vector<Source> *src, uint64_t first_job, uint64_t n_jobs, uint64_t n_ring,
              uint32_t n_readers, Opener *opener_or_null) {
        p = ctx->pool;
        R = n_ring ? n_ring : 1;
        base = first_job;
        end = first_job + n_jobs;
        next.store(first_job);
        opener = opener_or_null;
        return start_readers<Shared>(ctx, *this, cv, end, n_readers, [&] { filled.assign(n_jobs, 0); job_err.assign(n_jobs, 0); }, reader_main, jobs, src);
    }
    // Waits until job j has been read; meanwhile retires finished copies so that their buffers go back to the readers.  Returns
    // the errno of the job's read (0: fine).
    int wait(uint64_t j) {
        const int64_t k = (int64_t)(j - base);
        for (;;) {
            bool progress = false;
            while (copies_done < k && hipEventQuery(p->ev_copy[copies_done % R]) != hipErrorNotReady) { ++copies_done; progress = true; }   // (an error counts as done: the next HIP call reports it, nobody waits forever)
            std::unique_lock<std::mutex> lk(mu);
            if (progress) { freed = copies_done; lk.unlock(); cv.notify_all(); lk.lock(); }
            if (filled[k]) return job_err[k];
            cv.wait_for(lk, std::chrono::microseconds(copies_done < k ? 20 : 2000), [&] { return filled[k] != 0; });
            if (filled[k]) return job_err[k];
        }
    }
    void *staging(uint64_t j) const { return p->staging[(j - base) % R]; }
    hipEvent_t copy_event(uint64_t j) const { return p->ev_copy[(j - base) % R]; }
    hipStream_t copy_stream(uint64_t j) const { return (j & 1) ? p->copy_stream2 : p->copy_stream; }    // chunks alternate by job index
    // failed: the readers give up; otherwise they have read every job by now, or will.  Joins them either way.
    void stop(bool failed) { stop_readers<Shared>(*this, cv, end, failed); }
    ~Ring() { stop(true); }
};

struct DevScratch {                 // one carve-up of the context's scratch, shared by all files (the compute stream is in order)
    SampleDev *tables;              // [n_slots][table entries]
    size_t table_stride;            // bytes per slot
    uint64_t *totals, *site_line, *todo, *todo2, *status;
    uint32_t *todo_n;
    uint8_t *base, *filters;
    snpgpu_site_counts *counts;
    uint8_t *flag_rows;             // per slot: the site flags of its file (only with per-file exclude lists)
    size_t flag_row_stride;
};

// d_site_line: nullptr = in scratch; the single-pileup form passes the site set's own row, where
// snpgpu_siteset_line_offsets finds it afterwards.
// excl_off / excl_slots: nullptr, or per file the site-set slots of ITS exclude list (CSR, n_files + 1 offsets): the file is
// called with the set's flags | SNPGPU_SITE_EXCLUDED on those slots.
int run_stream(snpgpu_ctx *ctx, const snpgpu_siteset *ss, std::vector<Source> &src, const snpgpu_caller_params *prm,
               const Outputs &out, const snpgpu_stream_opts *opts, snpgpu_stream_stats *stats, uint64_t *d_site_line,
               const uint32_t *excl_off = nullptr, const uint32_t *excl_slots = nullptr, bool keep_spill = false) {
    const double t_start = now_s();
    const uint32_t n_files = (uint32_t)src.size();
    const uint32_t n_sites = ss->n_sites;
    if (stats) memset(stats, 0, sizeof *stats);
    if (!n_files) return SNPGPU_OK;
    if (excl_off) {
        if (excl_off[n_files] && !excl_slots) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "exclude slots missing");
        for (uint32_t f = 0; f < n_files; ++f) {
            if (excl_off[f + 1] < excl_off[f]) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "exclude offsets must be non-decreasing");
            for (uint32_t k = excl_off[f]; k < excl_off[f + 1]; ++k)
                if (excl_slots[k] >= n_sites) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "exclude slot %u of file %u is not in the site set", excl_slots[k], f);
        }
    }
    HIP_TRY(ctx, snpgpu_enter(ctx));
    if (out.counts && !keep_spill) { int rc0 = snpgpu_spill_begin(ctx); if (rc0) return rc0; }     // (keep_spill: one arena for several calls, begun by the caller)
    size_t chunk = opts && opts->chunk_bytes ? opts->chunk_bytes : (size_t)16 << 20;
    chunk = up(chunk < 65536 ? 65536 : chunk, SNPGPU_SCAN_TILE);
    const int want_depth = opts && opts->want_depth_sum ? 1 : 0;

    // ---- sources and jobs -------------------------------------------------------------------------------------
    uint64_t max_size = 0, total_bytes = 0;
    for (auto &s : src) {
        if (s.path) size_source(s);                             // (sized here, opened by the opener thread as the readers get to it)
        if (s.size > max_size && !s.dev) max_size = s.size;
        total_bytes += s.size;
    }
    Opener opener;
    auto close_all = [&]() { opener.finish(); for (auto &s2 : src) if (s2.fd >= 0) { close(s2.fd); s2.fd = -1; } };
    std::vector<Job> jobs;
    std::vector<uint32_t> chunks_of(n_files);
    uint32_t max_chunks = 1;
    for (uint32_t f = 0; f < n_files; ++f) {
        const uint64_t n = src[f].size;
        const uint32_t nc = n && !src[f].dev ? (uint32_t)((n + chunk - 1) / chunk) : 1;   // an empty file still takes one (empty) job, and so does device text
        chunks_of[f] = nc;
        if (nc > max_chunks) max_chunks = nc;
        for (uint32_t c = 0; c < nc; ++c) {
            const uint64_t off = (uint64_t)c * chunk;
            jobs.push_back(Job{f, off, src[f].dev ? 0 : (n - off < chunk ? n - off : chunk), c == 0, c + 1 == nc, c});
        }
    }
    const uint64_t J = jobs.size();
    opener.start(&src, chunks_of);                          // (the first files open while the staging memory is being pinned)

    // ---- resources ----------------------------------------------------------------------------------------------
    uint32_t n_readers, n_staging;                              // (the CPU budget of this process, not the box's CPU count)
    ring_sizes(J, opts && opts->n_readers ? opts->n_readers : snpgpu_reader_threads(), 4, &n_readers, &n_staging);
    if (opts && opts->n_staging) n_staging = (uint32_t)std::min<uint64_t>(opts->n_staging, J);
    uint32_t n_slots = opts && opts->n_slots ? opts->n_slots : 2;
    if (n_slots > n_files) n_slots = n_files;
    const size_t slot_bytes = up(max_size + SNPGPU_SCAN_TILE + 256, 4096);
    const size_t r_base = 0, r_filt = up(r_base + n_sites, 256), r_stat = up(r_filt + n_sites, 256), r_line = r_stat + 256;
    const bool to_dev = out.on_device;                          // (the rows of the block are then unused: it holds status words and flags)
    const size_t r_cnt = up(r_line + (out.line_off && !to_dev ? 8ull * n_sites : 0), 256);
    const size_t r_flags = up(r_cnt + (out.counts && !to_dev ? sizeof(snpgpu_site_counts) * (size_t)n_sites : 0), 256);
    const size_t result_bytes = r_flags + (excl_off ? up(n_sites, 256) : 0) + 256;
    const size_t table_bytes = up((size_t)(max_chunks + 1) * 2 * sizeof(SampleDev), 256);
    {
        int rc = pool_ensure(ctx, chunk, n_staging, n_slots, slot_bytes, result_bytes, table_bytes);
        if (rc) { close_all(); return rc; }
    }
    snpgpu_stream_pool *p = ctx->pool;                          // (it holds n_staging buffers or more: the ring uses n_staging)
    DevScratch ds;
    {
        const size_t list_bytes = up(8ull * n_sites, 256);
        size_t o = 0;
        const size_t o_tab = o; o += table_bytes * p->slot.size();
        const size_t o_tot = o; o += up(snpgpu_scan_totals_bytes(ctx), 256);
        const size_t o_line = o; o += list_bytes;
        const size_t o_todo = o; o += list_bytes;
        const size_t o_todo2 = o; o += list_bytes;
        const size_t o_base = o; o += up(n_sites, 256);
        const size_t o_filt = o; o += up(n_sites, 256);
        const size_t o_stat = o; o += 256;
        const size_t o_cnt = o; o += out.counts && !to_dev ? up(sizeof(snpgpu_site_counts) * (size_t)n_sites, 256) : 0;
        const size_t o_frow = o; o += excl_off ? up(n_sites, 256) * p->slot.size() : 0;
        void *ws = nullptr;
        int rc = snpgpu_scratch(ctx, o + 256, &ws);
        if (rc) { close_all(); return rc; }
        char *b = (char *)ws;
        ds.tables = (SampleDev *)(b + o_tab); ds.table_stride = table_bytes;
        ds.totals = (uint64_t *)(b + o_tot); ds.site_line = (uint64_t *)(b + o_line); ds.todo_n = snpgpu_call_ctl(ctx);
        if (!ds.todo_n) { close_all(); return SNPGPU_E_HIP; }
        ds.todo = (uint64_t *)(b + o_todo); ds.todo2 = (uint64_t *)(b + o_todo2); ds.base = (uint8_t *)(b + o_base);
        ds.filters = (uint8_t *)(b + o_filt); ds.status = (uint64_t *)(b + o_stat);
        ds.counts = out.counts && !to_dev ? (snpgpu_site_counts *)(b + o_cnt) : nullptr;
        ds.flag_rows = excl_off ? (uint8_t *)(b + o_frow) : nullptr;
        ds.flag_row_stride = up(n_sites, 256);
        if (d_site_line) ds.site_line = d_site_line;
    }
    hipStream_t st = ctx->stream;
    // whatever the caller enqueued before on the compute stream is done before the slots are overwritten
    {
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            close_all();
            return snpgpu_set_error(ctx, SNPGPU_E_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
        }
    }

    Ring ring;
    int rc = ring.start(ctx, &jobs, &src, 0, J, n_staging, n_readers, &opener);
    if (rc) { close_all(); return rc; }

    double t_wait_read = 0, t_wait_gpu = 0, t_enqueue = 0;
    auto harvest = [&](uint32_t f) -> int {                  // results of file f: pinned block -> the caller's arrays
        const uint32_t slot = f % (uint32_t)p->slot.size();
        const double t0 = now_s();
        hipError_t e = hipEventSynchronize(p->ev_done[slot]);
        t_wait_gpu += now_s() - t0;
        if (e != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "waiting for the results of pileup %u failed: %s", f, hipGetErrorString(e));
        const char *r = (const char *)p->result[slot];
        if (n_sites && !to_dev) {
            memcpy(out.base + (size_t)f * n_sites, r + r_base, n_sites);
            memcpy(out.filters + (size_t)f * n_sites, r + r_filt, n_sites);
            if (out.line_off) memcpy(out.line_off + (size_t)f * n_sites, r + r_line, 8ull * n_sites);
            if (out.counts) memcpy(out.counts + (size_t)f * n_sites, r + r_cnt, sizeof(snpgpu_site_counts) * (size_t)n_sites);
        }
        uint64_t *stw = out.status + (size_t)f * SNPGPU_SCAN_STATUS_WORDS;
        memcpy(stw, r + r_stat, 8 * SNPGPU_SCAN_STATUS_WORDS);
        if (src[f].rc == SNPGPU_OK && stw[0] != ~0ull)
            src[f].rc = (stw[0] & 0xFF) == SCAN_ERR_NON_ASCII ? SNPGPU_E_UNSUPPORTED : SNPGPU_E_PILEUP;
        return SNPGPU_OK;
    };
    {
        uint32_t harvested = 0;                              // files [0, harvested) have been copied out
        uint32_t cur_waves = 0;                              // waves of the final (whole-file) table entry of the current file
        uint32_t tiles_done = 0;
        for (uint64_t j = 0; j < J; ++j) {
            const Job &jb = jobs[j];
            const uint32_t f = jb.file, slot = f % (uint32_t)p->slot.size();
            Source &s = src[f];
            uint8_t *d_file = s.dev ? (uint8_t *)s.dev : (uint8_t *)p->slot[slot];
            SampleDev *h_tab = (SampleDev *)p->table_host[slot];
            SampleDev *d_tab = (SampleDev *)((char *)ds.tables + ds.table_stride * slot);
            const uint32_t nc = chunks_of[f];
            // where the kernels of this file leave their rows: the shared scratch rows (copied to the pinned block below), or row f
            // of the caller's device arrays (any byte alignment: the scan and the call kernels store per element)
            const size_t row = (size_t)f * n_sites;
            uint64_t *f_line = to_dev && out.line_off ? out.line_off + row : ds.site_line;
            uint8_t *f_base = to_dev ? out.base + row : ds.base, *f_filt = to_dev ? out.filters + row : ds.filters;
            snpgpu_site_counts *f_counts = to_dev && out.counts ? out.counts + row : ds.counts;
            if (jb.first) {
                // the slot, its table mirror and its result block are free once the file that used them has been harvested
                while (harvested + (uint32_t)p->slot.size() <= f) { rc = harvest(harvested); if (rc) goto done; ++harvested; }
                // one table entry (+ sentinel) per chunk: the part of the file that has landed after chunk c, and the tiles
                // that became complete with it; entry nc describes the whole file for the exact parser and the call step
                const uint64_t n_tiles = snpgpu_scan_tiles(d_file, s.size);
                uint32_t lo = 0;
                for (uint32_t c = 0; c <= nc; ++c) {
                    const bool whole = c + 1 >= nc;
                    const uint64_t landed = whole ? s.size : (uint64_t)(c + 1) * chunk;
                    SampleDev e{};
                    e.buf = d_file;
                    e.nbytes = landed;
                    e.status = ds.status;
                    e.tile_lo = c == nc ? 0 : lo;
                    e.tile_hi = whole ? (uint32_t)n_tiles : (uint32_t)((landed - SNPGPU_SCAN_HALO) / SNPGPU_SCAN_TILE);
                    if (c < nc) lo = e.tile_hi;
                    SampleDev sent{};
                    sent.wave0 = snpgpu_scan_deal(ctx, &e, 1, c == nc ? 1 : 8);
                    h_tab[2 * c] = e;
                    h_tab[2 * c + 1] = sent;
                }
                cur_waves = h_tab[2 * nc + 1].wave0;
                tiles_done = 0;
                STREAM_TRY(hipMemcpyAsync(d_tab, h_tab, (size_t)(nc + 1) * 2 * sizeof(SampleDev), hipMemcpyHostToDevice, st));
                rc = snpgpu_scan_begin(ctx, ss, d_tab + 2 * nc, 1, f_line, ds.todo_n, SNPGPU_CALL_PASSES - 1);
                if (rc) goto done;
            }
            {
                const double t0 = now_s();
                if (ring.wait(j) && s.rc == SNPGPU_OK) s.rc = SNPGPU_E_IO;
                t_wait_read += now_s() - t0;
            }
            const double t_e = now_s();
            hipStream_t cs = ring.copy_stream(j);
            if (jb.len) STREAM_TRY(hipMemcpyAsync(d_file + jb.off, ring.staging(j), jb.len, hipMemcpyHostToDevice, cs));
            STREAM_TRY(hipEventRecord(ring.copy_event(j), cs));
            STREAM_TRY(hipStreamWaitEvent(st, ring.copy_event(j), 0));
            const SampleDev &e = h_tab[2 * jb.chunk];
            if (e.tile_hi > tiles_done) {
                rc = snpgpu_scan_range(ctx, ss, d_tab + 2 * jb.chunk, 1, h_tab[2 * jb.chunk + 1].wave0, ds.totals, f_line, want_depth);
                if (rc) goto done;
                tiles_done = e.tile_hi;
            }
            if (jb.last) {
                const SampleDev *d_whole = d_tab + 2 * nc;
                rc = snpgpu_scan_end(ctx, ss, d_whole, 1, cur_waves, ds.totals, f_line, want_depth);
                char *r = (char *)p->result[slot];
                const uint8_t *d_flags = nullptr;
                if (rc == SNPGPU_OK && excl_off && n_sites) {
                    // this file's site flags: the set's, with its own exclude list on top (the pinned row is free: the file that
                    // used this block before has been harvested)
                    uint8_t *hf = (uint8_t *)(r + r_flags);
                    memcpy(hf, ss->h_flags.data(), n_sites);
                    for (uint32_t k = excl_off[f]; k < excl_off[f + 1]; ++k) hf[excl_slots[k]] |= SNPGPU_SITE_EXCLUDED;
                    uint8_t *d_row = ds.flag_rows + ds.flag_row_stride * slot;
                    STREAM_TRY(hipMemcpyAsync(d_row, hf, n_sites, hipMemcpyHostToDevice, st));
                    d_flags = d_row;
                }
                if (rc == SNPGPU_OK)
                    rc = snpgpu_enqueue_call(ctx, ss, d_whole, 1, prm, f_line, f_base, f_filt, f_counts, ds.todo_n, ds.todo, ds.todo2,
                                             d_flags, 0);
                if (rc) goto done;
                if (to_dev && n_sites && s.rc == SNPGPU_E_IO) {
                    // could not be opened or read (known by now: the last piece has been waited for): its rows are void, and in the
                    // caller's arrays that is '-' / 0 / no line / zeroed records rather than whatever the pieces that did arrive gave
                    STREAM_TRY(hipMemsetAsync(f_base, '-', n_sites, st));
                    STREAM_TRY(hipMemsetAsync(f_filt, 0, n_sites, st));
                    if (out.line_off) STREAM_TRY(hipMemsetAsync(f_line, 0, 8ull * n_sites, st));
                    if (out.counts) STREAM_TRY(hipMemsetAsync(f_counts, 0, sizeof(snpgpu_site_counts) * (size_t)n_sites, st));
                }
                if (n_sites && !to_dev) {
                    STREAM_TRY(hipMemcpyAsync(r + r_base, ds.base, n_sites, hipMemcpyDeviceToHost, st));
                    STREAM_TRY(hipMemcpyAsync(r + r_filt, ds.filters, n_sites, hipMemcpyDeviceToHost, st));
                    if (out.line_off) STREAM_TRY(hipMemcpyAsync(r + r_line, ds.site_line, 8ull * n_sites, hipMemcpyDeviceToHost, st));
                    if (out.counts) STREAM_TRY(hipMemcpyAsync(r + r_cnt, ds.counts, sizeof(snpgpu_site_counts) * (size_t)n_sites, hipMemcpyDeviceToHost, st));
                }
                STREAM_TRY(hipMemcpyAsync(r + r_stat, ds.status, 8 * SNPGPU_SCAN_STATUS_WORDS, hipMemcpyDeviceToHost, st));
                // (the next file that uses this slot is not started before this event has been waited for in harvest())
                STREAM_TRY(hipEventRecord(p->ev_done[slot], st));
            }
            t_enqueue += now_s() - t_e;
        }
        while (harvested < n_files) { rc = harvest(harvested); if (rc) goto done; ++harvested; }
    }
done:
    ring.stop(rc != SNPGPU_OK);
    if (rc) { (void)hipStreamSynchronize(p->copy_stream); (void)hipStreamSynchronize(p->copy_stream2); (void)hipStreamSynchronize(st); }
    close_all();
    if (out.rc) for (uint32_t f = 0; f < n_files; ++f) out.rc[f] = src[f].rc;
    if (stats) {
        stats->bytes = total_bytes;
        stats->seconds = now_s() - t_start;
        stats->seconds_waiting_for_readers = t_wait_read;
        stats->seconds_waiting_for_device = t_wait_gpu;
        stats->n_chunks = J;
        stats->n_readers = n_readers;
        stats->n_staging = n_staging;
        stats->chunk_bytes = (uint32_t)chunk;
        stats->reader_seconds_reading = ring.ns_reading.load() * 1e-9;
        stats->reader_seconds_waiting = ring.ns_waiting.load() * 1e-9;
        stats->seconds_enqueueing = t_enqueue;
    }
    return rc;
}

// One file into device slot 0 through the same reader threads / staging ring / two copy streams as run_stream (the
// all-lines passes: --vcfAllPos and phase-1 site calling index the whole file before they look at a line, so there is
// nothing to overlap the copy with but the reads).  Synchronous.
// n_slots / min_slot_bytes: what the pool must hold besides (a BGZF file: a second slot, both large enough for the text).
int load_raw(snpgpu_ctx *ctx, const char *path, uint32_t n_slots, size_t min_slot_bytes, uint8_t **d_file, uint64_t *size) {
    std::vector<Source> src(1);
    Source &s = src[0];
    s.path = path;
    s.fd = open(path, O_RDONLY | O_CLOEXEC);
    struct stat stt;
    if (s.fd < 0 || fstat(s.fd, &stt) != 0 || !S_ISREG(stt.st_mode)) {
        if (s.fd >= 0) close(s.fd);
        return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot open the pileup file %s", path);
    }
    const uint64_t n = s.size = (uint64_t)stt.st_size;
    (void)posix_fadvise(s.fd, 0, 0, POSIX_FADV_SEQUENTIAL);
    const size_t chunk = (size_t)16 << 20;
    std::vector<Job> jobs;
    for (uint64_t off = 0, c = 0; off < n; ++c) {                // 1, 1, 2, 4, 8, 16, 16, ... MiB
        const uint64_t want = ramp_piece(c, chunk), len = n - off < want ? n - off : want;
        jobs.push_back(Job{0, off, len, c == 0, off + len >= n, (uint32_t)c});
        off += len;
    }
    const uint64_t J = jobs.size();
    uint32_t n_readers, n_staging;
    ring_sizes(J, snpgpu_reader_threads(), 4, &n_readers, &n_staging);
    size_t slot_bytes = up(n + SNPGPU_SCAN_TILE + 256, 4096);
    if (slot_bytes < min_slot_bytes) slot_bytes = min_slot_bytes;
    int rc = pool_ensure(ctx, chunk, n_staging, n_slots, slot_bytes, 256, 256);
    if (rc) { close(s.fd); return rc; }
    snpgpu_stream_pool *p = ctx->pool;
    uint8_t *d = (uint8_t *)p->slot[0];
    hipError_t he = hipStreamSynchronize(ctx->stream);          // earlier work on the slot is done
    Ring ring;
    bool io_failed = false;
    if (he == hipSuccess && J) {
        rc = ring.start(ctx, &jobs, &src, 0, J, n_staging, n_readers, nullptr);
        if (rc) { close(s.fd); return rc; }
        for (uint64_t j = 0; j < J && he == hipSuccess; ++j) {
            if (ring.wait(j)) io_failed = true;
            hipStream_t cs = ring.copy_stream(j);
            he = hipMemcpyAsync(d + jobs[j].off, ring.staging(j), jobs[j].len, hipMemcpyHostToDevice, cs);
            if (he == hipSuccess) he = hipEventRecord(ring.copy_event(j), cs);
        }
        ring.stop(he != hipSuccess);
        hipError_t e1 = hipStreamSynchronize(p->copy_stream), e2 = hipStreamSynchronize(p->copy_stream2);
        if (he == hipSuccess) he = e1 != hipSuccess ? e1 : e2;
    }
    close(s.fd);
    if (he != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "loading %s failed: %s", path, hipGetErrorString(he));
    if (io_failed) return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot read the pileup file %s", path);
    *d_file = d;
    *size = n;
    return SNPGPU_OK;
}

// A BGZF file: its block table from a header-hopping pass over the mapped file, its compressed bytes into slot 0 the same way,
// the inflate kernel from there into slot 1 (sized from the table, never from the compressed size).  Synchronous; the text stays
// valid until the next call that loads a file.  info (nullable) says which block was bad and why.
int load_bgzf(snpgpu_ctx *ctx, const char *path, uint8_t **d_file, uint64_t *size, snpgpu_bgzf_info *info) {
    snpgpu_bgzf_info local;
    if (!info) info = &local;
    std::vector<snpgpu_bgzf_block> blocks;
    const uint8_t *map = nullptr;
    uint64_t map_bytes = 0;
    int rc = snpgpu_bgzf_index_file(path, blocks, info, &map, &map_bytes);
    if (map) munmap((void *)map, map_bytes);
    if (rc == SNPGPU_E_IO) return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot open the pileup file %s", path);
    if (rc != SNPGPU_OK)
        return snpgpu_set_error(ctx, rc == SNPGPU_BGZF_E_TRUNCATED ? SNPGPU_E_IO : rc == SNPGPU_BGZF_E_NOT_BGZF || rc == SNPGPU_BGZF_E_NOT_GZIP ? SNPGPU_E_UNSUPPORTED : SNPGPU_E_PILEUP,
                                "compressed pileup %s: %s (block %llu at byte offset %llu)", path, snpgpu_bgzf_strerror(rc), (unsigned long long)info->bad_block,
                                (unsigned long long)info->bad_offset);
    const uint64_t plain = info->plain_bytes;
    uint8_t *d_comp = nullptr;
    uint64_t n_comp = 0;
    rc = load_raw(ctx, path, 2, up(plain + SNPGPU_SCAN_TILE + 256, 4096), &d_comp, &n_comp);
    if (rc == SNPGPU_E_NOMEM) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "no device memory for the %llu bytes of text of the compressed pileup %s", (unsigned long long)plain, path);
    if (rc) return rc;
    if (n_comp != info->compressed_bytes) return snpgpu_set_error(ctx, SNPGPU_E_IO, "the pileup file %s changed while it was read", path);
    uint8_t *d_text = (uint8_t *)ctx->pool->slot[1];
    rc = snpgpu_bgzf_check_table(ctx, blocks.data(), blocks.size(), n_comp, plain);
    if (rc) return rc;
    void *ws = nullptr;
    rc = snpgpu_scratch(ctx, snpgpu_bgzf_scratch_bytes(blocks.size()), &ws);
    if (rc) return rc;
    uint32_t *d_status = nullptr;
    rc = snpgpu_enqueue_bgzf_inflate(ctx, d_comp, blocks.data(), blocks.size(), d_text, ws, &d_status);
    if (rc) return rc;
    std::vector<uint32_t> st(blocks.size());
    if (!st.empty()) HIP_TRY(ctx, hipMemcpyAsync(st.data(), d_status, 4 * st.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    snpgpu_bgzf_summarise(blocks.data(), st.data(), blocks.size(), info);
    if (info->n_bad)
        return snpgpu_set_error(ctx, SNPGPU_E_PILEUP, "compressed pileup %s: block %llu at byte offset %llu: %s", path, (unsigned long long)info->bad_block,
                                (unsigned long long)info->bad_offset, snpgpu_bgzf_status_name(info->bad_status));
    *d_file = d_text;
    *size = plain;
    return SNPGPU_OK;
}

// The text of a pileup file in device memory, whether the file holds it plain or BGZF-compressed (decided by content).
int load_file(snpgpu_ctx *ctx, const char *path, uint8_t **d_file, uint64_t *size) {
    const int kind = snpgpu_bgzf_probe(path);
    if (kind == 1) return load_bgzf(ctx, path, d_file, size, nullptr);
    if (kind == SNPGPU_BGZF_E_NOT_BGZF || kind == SNPGPU_BGZF_E_TRUNCATED || kind == SNPGPU_BGZF_E_MAGIC)
        return snpgpu_set_error(ctx, kind == SNPGPU_BGZF_E_TRUNCATED ? SNPGPU_E_IO : SNPGPU_E_UNSUPPORTED, "compressed pileup %s: %s", path, snpgpu_bgzf_strerror(kind));
    return load_raw(ctx, path, 1, 0, d_file, size);         // (a file that cannot be opened fails there, in the words it always did)
}

int scan_status_error(snpgpu_ctx *ctx, const uint64_t *status, const char *what_file) {
    unsigned code = (unsigned)(status[0] & 0xFF);
    unsigned long long off = (unsigned long long)(status[0] >> 8) - 1;
    const char *what = code == SCAN_ERR_FEW_FIELDS ? "line has fewer than 2 fields" :
                       code == SCAN_ERR_BAD_POS ? "position field is not an unsigned decimal integer" :
                       code == SCAN_ERR_NON_ASCII ? "non-ASCII byte" : "malformed line";
    return snpgpu_set_error(ctx, code == SCAN_ERR_NON_ASCII ? SNPGPU_E_UNSUPPORTED : SNPGPU_E_PILEUP,
                            "pileup%s%s: %s at byte offset %llu", what_file ? " " : "", what_file ? what_file : "", what, off);
}

}  // namespace

extern "C" {

int snpgpu_call_consensus_files(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const char *const *paths, uint32_t n_files,
                                const snpgpu_caller_params *params, const uint32_t *excl_off, const uint32_t *excl_slots,
                                uint8_t *out_base, uint8_t *out_filters,
                                snpgpu_site_counts *out_counts, uint64_t *out_line_off, uint64_t *out_status,
                                int32_t *out_rc, const snpgpu_stream_opts *opts, snpgpu_stream_stats *stats) {
    if (!ctx || !ss || !params || !out_status || (n_files && !paths)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (ss->n_sites && n_files && (!out_base || !out_filters)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null output");
    std::vector<Source> src(n_files);
    for (uint32_t f = 0; f < n_files; ++f) {
        if (!paths[f]) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null path %u", f);
        src[f].path = paths[f];
    }
    Outputs out{out_base, out_filters, out_counts, out_line_off, out_status, out_rc};
    return run_stream(ctx, ss, src, params, out, opts, stats, nullptr, excl_off, excl_slots);
}

// The same stream with the rows left on the device: the kernels of file f write row f of the caller's [n_files][n_sites] arrays
// (the layout of snpgpu_call_consensus_many_dev), so a group of samples that was never resident is ready for the flow kernels
// when the call returns.  Status words and return codes come back on the host, per file, as above.
int snpgpu_call_consensus_files_dev(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const char *const *paths, uint32_t n_files,
                                    const snpgpu_caller_params *params, const uint32_t *excl_off, const uint32_t *excl_slots,
                                    uint8_t *d_out_base, uint8_t *d_out_filters,
                                    snpgpu_site_counts *d_out_counts, uint64_t *d_out_line_off, uint64_t *out_status,
                                    int32_t *out_rc, const snpgpu_stream_opts *opts, snpgpu_stream_stats *stats) {
    if (!ctx || !ss || !params || !out_status || (n_files && !paths)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (ss->n_sites && n_files && (!d_out_base || !d_out_filters)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null output");
    std::vector<Source> src(n_files);
    for (uint32_t f = 0; f < n_files; ++f) {
        if (!paths[f]) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null path %u", f);
        src[f].path = paths[f];
    }
    Outputs out{d_out_base, d_out_filters, d_out_counts, d_out_line_off, out_status, out_rc};
    out.on_device = true;
    return run_stream(ctx, ss, src, params, out, opts, stats, nullptr, excl_off, excl_slots);
}

// BGZF files: each one is loaded and inflated (load_bgzf), then takes the whole-file sequence of the stream above as text that is
// already on the device.  One file at a time: the read, copy and inflate of a file do not yet overlap the scan and call of the one before.
int snpgpu_call_consensus_bgzf_files(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const char *const *paths, uint32_t n_files,
                                     const snpgpu_caller_params *params, const uint32_t *excl_off, const uint32_t *excl_slots,
                                     uint8_t *out_base, uint8_t *out_filters,
                                     snpgpu_site_counts *out_counts, uint64_t *out_line_off, uint64_t *out_status,
                                     int32_t *out_rc, const snpgpu_stream_opts *opts, snpgpu_stream_stats *stats, snpgpu_bgzf_info *out_info) {
    if (!ctx || !ss || !params || !out_status || (n_files && !paths)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (ss->n_sites && n_files && (!out_base || !out_filters)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null output");
    for (uint32_t f = 0; f < n_files; ++f) if (!paths[f]) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null path %u", f);
    const double t_start = now_s();
    if (stats) memset(stats, 0, sizeof *stats);
    HIP_TRY(ctx, snpgpu_enter(ctx));
    const size_t n_sites = ss->n_sites;
    if (out_counts) { int rc0 = snpgpu_spill_begin(ctx); if (rc0) return rc0; }     // the spill records of all files of the call form one arena
    std::string first_error;
    uint64_t total = 0;
    for (uint32_t f = 0; f < n_files; ++f) {
        uint8_t *d_text = nullptr;
        uint64_t nbytes = 0;
        const size_t row = (size_t)f * n_sites;
        int rc = load_bgzf(ctx, paths[f], &d_text, &nbytes, out_info ? out_info + f : nullptr);
        if (rc == SNPGPU_E_HIP || rc == SNPGPU_E_NOMEM || rc == SNPGPU_E_ARG) return rc;
        if (rc == SNPGPU_OK) {
            std::vector<Source> src(1);
            src[0].dev = d_text;
            src[0].size = nbytes;
            Outputs out{out_base + row, out_filters + row, out_counts ? out_counts + row : nullptr, out_line_off ? out_line_off + row : nullptr,
                        out_status + (size_t)f * SNPGPU_SCAN_STATUS_WORDS, out_rc ? out_rc + f : nullptr};
            snpgpu_stream_stats one;
            rc = run_stream(ctx, ss, src, params, out, opts, &one, nullptr, excl_off ? excl_off + f : nullptr, excl_slots, true);
            if (rc) return rc;
            total += nbytes;
            if (stats) { stats->n_chunks += 1; stats->seconds_waiting_for_device += one.seconds_waiting_for_device; stats->seconds_enqueueing += one.seconds_enqueueing; }
            continue;
        }
        // this file has no text: its rows are void, the others go on
        if (first_error.empty()) first_error = ctx->err;
        if (n_sites) {
            memset(out_base + row, '-', n_sites);
            memset(out_filters + row, 0, n_sites);
            if (out_counts) memset(out_counts + row, 0, sizeof(snpgpu_site_counts) * n_sites);
            if (out_line_off) memset(out_line_off + row, 0, 8 * n_sites);
        }
        uint64_t *stw = out_status + (size_t)f * SNPGPU_SCAN_STATUS_WORDS;
        memset(stw, 0, 8 * SNPGPU_SCAN_STATUS_WORDS);
        stw[0] = ~0ull;
        if (out_rc) out_rc[f] = rc;
    }
    if (!first_error.empty()) ctx->err = first_error;       // (snpgpu_last_error: the first file that failed, with its block and cause)
    if (stats) { stats->bytes = total; stats->seconds = now_s() - t_start; }
    return SNPGPU_OK;
}

// Host-buffer form for ONE pileup (an mmap, bytes read elsewhere): same pipeline, the readers memcpy instead of pread.
// Synchronous.  Returns SNPGPU_E_PILEUP / SNPGPU_E_UNSUPPORTED when the scan found a malformed line (status words still filled).
int snpgpu_call_consensus(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const uint8_t *pileup, size_t nbytes,
                          const snpgpu_caller_params *params, uint8_t *out_base, uint8_t *out_filters,
                          snpgpu_site_counts *out_counts, uint64_t *out_status, int want_depth_sum) {
    if (!ctx || !ss || !params || !out_status || (nbytes && !pileup)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (ss->n_sites && (!out_base || !out_filters)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null output");
    static const uint8_t empty = 0;
    std::vector<Source> src(1);
    src[0].mem = nbytes ? pileup : &empty;
    src[0].size = nbytes;
    snpgpu_stream_opts o{};
    o.want_depth_sum = want_depth_sum ? 1u : 0u;
    Outputs out{out_base, out_filters, out_counts, nullptr, out_status, nullptr};
    int rc = run_stream(ctx, ss, src, params, out, &o, nullptr, ss->site_line);
    if (rc) return rc;
    if (out_status[0] != ~0ull) return scan_status_error(ctx, out_status, nullptr);
    return SNPGPU_OK;
}

}  // extern "C"

namespace {

// The all-lines pass on the device (--vcfAllPos): the file into device memory, its line index, a record per line.  What it leaves
// behind lives in the context's scratch (valid until the next call that takes scratch); nothing has been copied back but the number
// of lines.  With `compact`: also the 24-byte records and the count of the wide ones (lines_out.hip).
struct AllLines {
    uint8_t *d_file = nullptr;
    uint64_t nbytes = 0;
    uint32_t n_lines = 0;
    uint64_t *d_off = nullptr;
    uint8_t *d_flags = nullptr;
    snpgpu_site_counts *d_counts = nullptr;
    uint64_t *d_status = nullptr;
    snpgpu_line_record *d_recs = nullptr;       // compact only
    uint32_t *d_compact_ws = nullptr, *d_n_wide = nullptr;
    uint32_t *d_wide_index = nullptr;           // room for n_lines of each: the gather's targets
    snpgpu_site_counts *d_wide = nullptr;
};

// Returns SNPGPU_OK with al.n_lines set; when n_lines == 0 or n_lines > capacity nothing else has been done (al.d_counts == nullptr).
int all_lines_pass(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const char *path, const snpgpu_caller_params *params, uint64_t capacity, bool compact,
                   AllLines &al) {
    int rc = snpgpu_spill_begin(ctx);
    if (rc) return rc;
    rc = load_file(ctx, path, &al.d_file, &al.nbytes);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const uint8_t *d_file = al.d_file;
    const uint64_t nbytes = al.nbytes;
    const size_t ws_words = snpgpu_lines_workspace_words(nbytes);
    // first the count alone (its workspace is all the scratch it needs) ...
    void *scr = nullptr;
    rc = snpgpu_scratch(ctx, up(4 * ws_words, 256) + 512, &scr);
    if (rc) return rc;
    uint32_t *d_total = nullptr;
    rc = snpgpu_enqueue_lines_count(ctx, d_file, nbytes, (uint32_t *)scr, &d_total);
    if (rc) return rc;
    uint32_t n_lines = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n_lines, d_total, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    al.n_lines = n_lines;
    if (n_lines > capacity || n_lines == 0) return SNPGPU_OK;
    // ... then everything: the scratch may move, so the count is redone in the new place (cheap next to the call step)
    size_t o = up(4 * ws_words, 256);
    const size_t o_off = o; o += up(8ull * n_lines, 256);
    const size_t o_flag = o; o += up(n_lines, 256);
    const size_t o_base = o; o += up(n_lines, 256);
    const size_t o_filt = o; o += up(n_lines, 256);
    const size_t o_stat = o; o += 256;
    const size_t o_samp = o; o += 256;
    const size_t o_cnt = o; o += up(sizeof(snpgpu_site_counts) * (size_t)n_lines, 256);
    const size_t o_todo = o; o += 2 * up(8ull * n_lines, 256) + 256;           // the lane kernels' leftover lists and their counts
    const size_t o_rec = o; if (compact) o += up(sizeof(snpgpu_line_record) * (size_t)n_lines, 256);
    const size_t o_cws = o; if (compact) o += up(4 * snpgpu_compact_lines_workspace_words(n_lines), 256);
    const size_t o_widx = o; if (compact) o += up(4ull * n_lines, 256);
    const size_t o_wide = o; if (compact) o += up(sizeof(snpgpu_site_counts) * (size_t)n_lines, 256);     // (every line may be wide; 288 GB of HBM)
    rc = snpgpu_scratch(ctx, o + 256, &scr);
    if (rc) return rc;
    char *b = (char *)scr;
    rc = snpgpu_enqueue_lines_count(ctx, d_file, nbytes, (uint32_t *)b, &d_total);
    if (rc) return rc;
    uint64_t h_status[SNPGPU_SCAN_STATUS_WORDS] = {~0ull, n_lines, 0, 0};
    SampleDev sd{};
    sd.buf = d_file;
    sd.nbytes = nbytes;
    sd.status = (uint64_t *)(b + o_stat);
    HIP_TRY(ctx, hipMemcpyAsync(b + o_stat, h_status, sizeof h_status, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(b + o_samp, &sd, sizeof sd, hipMemcpyHostToDevice, st));
    rc = snpgpu_enqueue_lines_emit(ctx, ss, d_file, nbytes, (uint32_t *)b, (uint64_t *)(b + o_off), (uint8_t *)(b + o_flag), n_lines,
                                   (uint64_t *)(b + o_stat));
    if (rc == SNPGPU_OK)
        rc = snpgpu_enqueue_call_lines(ctx, (const SampleDev *)(b + o_samp), (const uint64_t *)(b + o_off), (const uint8_t *)(b + o_flag),
                                       n_lines, params, (uint8_t *)(b + o_base), (uint8_t *)(b + o_filt), (snpgpu_site_counts *)(b + o_cnt),
                                       snpgpu_call_ctl(ctx), (uint64_t *)(b + o_todo + 256), (uint64_t *)(b + o_todo + 256 + up(8ull * n_lines, 256)));
    if (rc) return rc;
    al.d_off = (uint64_t *)(b + o_off);
    al.d_flags = (uint8_t *)(b + o_flag);
    al.d_counts = (snpgpu_site_counts *)(b + o_cnt);
    al.d_status = (uint64_t *)(b + o_stat);
    if (compact) {
        al.d_recs = (snpgpu_line_record *)(b + o_rec);
        al.d_compact_ws = (uint32_t *)(b + o_cws);
        al.d_wide_index = (uint32_t *)(b + o_widx);
        al.d_wide = (snpgpu_site_counts *)(b + o_wide);
        rc = snpgpu_enqueue_compact_lines(ctx, al.d_counts, al.d_flags, n_lines, al.d_recs, al.d_compact_ws, &al.d_n_wide);
    }
    return rc;
}

}  // namespace

extern "C" {

// call_consensus --vcfAllPos (call_consensus.py:148-151, pileup.py:418-421): a Record for EVERY line of the pileup.
// Synchronous, host outputs in file order: out_line_off[i] = 1 + byte offset of line i, out_line_flags[i] = SNPGPU_SITE_*
// of its position (0 when it is not in the site set), out_counts[i] its record.  *out_n_lines is always set; when it
// exceeds `capacity` nothing else is written and the caller comes back with larger arrays.  out_status: scan status words
// ([0] = first line whose chrom / position columns are malformed, [1] = number of lines).
int snpgpu_call_all_lines_file(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const char *path, const snpgpu_caller_params *params,
                               uint64_t capacity, uint64_t *out_n_lines, uint64_t *out_line_off, uint8_t *out_line_flags,
                               snpgpu_site_counts *out_counts, uint64_t *out_status) {
    if (!ctx || !ss || !path || !params || !out_n_lines || !out_status) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (capacity && (!out_line_off || !out_line_flags || !out_counts)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null output");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    AllLines al;
    int rc = all_lines_pass(ctx, ss, path, params, capacity, false, al);
    if (rc) return rc;
    const uint32_t n_lines = al.n_lines;
    *out_n_lines = n_lines;
    out_status[0] = ~0ull; out_status[1] = n_lines; out_status[2] = out_status[3] = 0;
    if (!al.d_counts) return SNPGPU_OK;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(out_line_off, al.d_off, 8ull * n_lines, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_line_flags, al.d_flags, n_lines, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_counts, al.d_counts, sizeof(snpgpu_site_counts) * (size_t)n_lines, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_status, al.d_status, 8 * SNPGPU_SCAN_STATUS_WORDS, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    out_status[1] = n_lines;
    if (out_status[0] != ~0ull) return scan_status_error(ctx, out_status, path);
    return SNPGPU_OK;
}

// The same with 24-byte records: see include/snpgpu.h.
int snpgpu_call_all_lines_compact_file(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const char *path, const snpgpu_caller_params *params,
                                       uint64_t capacity, uint64_t *out_n_lines, uint64_t *out_line_off, snpgpu_line_record *out_records,
                                       uint32_t wide_capacity, uint32_t *out_n_wide, uint32_t *out_wide_index, snpgpu_site_counts *out_wide,
                                       uint64_t *out_status) {
    if (!ctx || !ss || !path || !params || !out_n_lines || !out_n_wide || !out_status) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (capacity && (!out_line_off || !out_records)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null output");
    if (wide_capacity && (!out_wide_index || !out_wide)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null output");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    AllLines al;
    int rc = all_lines_pass(ctx, ss, path, params, capacity, true, al);
    if (rc) return rc;
    const uint32_t n_lines = al.n_lines;
    *out_n_lines = n_lines;
    *out_n_wide = 0;
    out_status[0] = ~0ull; out_status[1] = n_lines; out_status[2] = out_status[3] = 0;
    if (!al.d_counts) return SNPGPU_OK;
    hipStream_t st = ctx->stream;
    uint32_t n_wide = 0;
    // the bulk goes while the host learns how many wide lines there are
    HIP_TRY(ctx, hipMemcpyAsync(&n_wide, al.d_n_wide, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_status, al.d_status, 8 * SNPGPU_SCAN_STATUS_WORDS, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *out_n_wide = n_wide;
    out_status[1] = n_lines;
    if (out_status[0] != ~0ull) return scan_status_error(ctx, out_status, path);
    if (n_wide > wide_capacity) return SNPGPU_OK;                 // the caller comes back with room for them
    HIP_TRY(ctx, hipMemcpyAsync(out_line_off, al.d_off, 8ull * n_lines, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_records, al.d_recs, sizeof(snpgpu_line_record) * (size_t)n_lines, hipMemcpyDeviceToHost, st));
    if (n_wide) {
        rc = snpgpu_enqueue_gather_wide(ctx, al.d_counts, al.d_recs, n_lines, al.d_compact_ws, n_wide, al.d_wide_index, al.d_wide);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(out_wide_index, al.d_wide_index, 4ull * n_wide, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(out_wide, al.d_wide, sizeof(snpgpu_site_counts) * (size_t)n_wide, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return SNPGPU_OK;
}

// --vcfAllPos from file to file: see include/snpgpu.h.  The records come back in pieces into pinned memory while host threads format the
// rows of the pieces that have landed; the pileup's own text (CHROM and POS of every row) is read through a private mapping of the file,
// which the load has just pulled into the page cache.
int snpgpu_write_all_positions_vcf(snpgpu_ctx *ctx, const snpgpu_siteset *ss, const char *pileup_path, const snpgpu_caller_params *params,
                                   const char *vcf_path, const char *header, const char *const *filter_names, int preserve_ref_case,
                                   char failed_snp_gt, int only_listed, int check, uint64_t *out_n_lines, uint64_t *out_n_rows,
                                   uint64_t *out_first_bad_line, uint64_t *out_first_bad_off, snpgpu_site_counts *out_first_bad, uint64_t *out_status) {
    if (!ctx || !ss || !pileup_path || !params || !vcf_path || !header || !filter_names || !out_n_lines || !out_n_rows || !out_first_bad_line ||
        !out_first_bad_off || !out_first_bad || !out_status)
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    // the rows are formatted from the pileup's text on the host: a compressed pileup is refused before anything is opened or truncated
    if (snpgpu_bgzf_probe(pileup_path) == 1)
        return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "every-position VCF output from a BGZF-compressed pileup is not supported: %s", pileup_path);
    HIP_TRY(ctx, snpgpu_enter(ctx));
    *out_n_lines = *out_n_rows = 0;
    *out_first_bad_line = ~0ull;
    *out_first_bad_off = 0;
    hipStream_t st = ctx->stream;
    AllLines al;
    uint32_t n_lines = 0, n_wide = 0, n_spill = 0;
    bool scan_bad = false;
    std::vector<snpgpu_symbol_spill> spill;
    for (int attempt = 0;; ++attempt) {                          // (again when the positions asked for more spill records than the arena held)
        al = AllLines();
        int rc = all_lines_pass(ctx, ss, pileup_path, params, ~0ull, true, al);
        if (rc) return rc;
        n_lines = al.n_lines;
        *out_n_lines = n_lines;
        out_status[0] = ~0ull; out_status[1] = n_lines; out_status[2] = out_status[3] = 0;
        if (!al.d_counts) break;                                 // an empty file: the header alone
        HIP_TRY(ctx, hipMemcpyAsync(&n_wide, al.d_n_wide, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(&n_spill, ctx->d_spill_n, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(out_status, al.d_status, 8 * SNPGPU_SCAN_STATUS_WORDS, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        out_status[1] = n_lines;
        scan_bad = out_status[0] != ~0ull;       // (reported below, after a look for an earlier line that a Record cannot be built from)
        if (scan_bad || n_spill <= ctx->spill_cap) break;
        if (attempt >= 4 || n_spill > 0xFFFFFEu) return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "%u lines of %s need a spill record", n_spill, pileup_path);
        const uint64_t want = (uint64_t)n_spill + n_spill / 4 + 64;
        ctx->spill_want = want > 0xFFFFFEull ? 0xFFFFFEu : (uint32_t)want;
    }
    // the wide lines (few) and the spill records they point at: all at once
    std::vector<uint32_t> wide_index(n_wide);
    std::vector<snpgpu_site_counts> wide(n_wide);
    if (al.d_counts && n_wide) {
        int rc = snpgpu_enqueue_gather_wide(ctx, al.d_counts, al.d_recs, n_lines, al.d_compact_ws, n_wide, al.d_wide_index, al.d_wide);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(wide_index.data(), al.d_wide_index, 4ull * n_wide, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(wide.data(), al.d_wide, sizeof(snpgpu_site_counts) * (size_t)n_wide, hipMemcpyDeviceToHost, st));
        if (n_spill > ctx->spill_cap) n_spill = ctx->spill_cap;
        spill.resize(n_spill);
        if (n_spill) HIP_TRY(ctx, hipMemcpyAsync(spill.data(), ctx->d_spill, sizeof(snpgpu_symbol_spill) * (size_t)n_spill, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (check)
            for (uint32_t k = 0; k < n_wide; ++k)
                if (wide[k].status > SNPGPU_ST_OK) {             // the first line a Record cannot be built from: the caller raises, nothing is written
                    *out_first_bad_line = wide_index[k];
                    *out_first_bad = wide[k];
                    HIP_TRY(ctx, hipMemcpy(out_first_bad_off, al.d_off + wide_index[k], 8, hipMemcpyDeviceToHost));
                    break;
                }
    }
    if (scan_bad) return scan_status_error(ctx, out_status, pileup_path);
    if (*out_first_bad_line != ~0ull) return SNPGPU_OK;
    // the pileup's text for CHROM / POS
    const uint8_t *text = nullptr;
    int pfd = -1;
    if (n_lines) {
        pfd = open(pileup_path, O_RDONLY | O_CLOEXEC);
        void *m = pfd >= 0 ? mmap(nullptr, al.nbytes, PROT_READ, MAP_PRIVATE, pfd, 0) : MAP_FAILED;
        if (m == MAP_FAILED) { if (pfd >= 0) close(pfd); return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot map the pileup file %s", pileup_path); }
        text = (const uint8_t *)m;
    }
    const int vfd = open(vcf_path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    std::atomic<bool> io_ok{vfd >= 0};
    const size_t header_len = strlen(header);
    // pieces of lines: offsets + records of a piece come back into one pinned buffer each (two copies on the stream, an event behind
    // them); a pool of threads takes the pieces in order, formats, and writes its text at the offset the pieces before it end at
    const uint64_t piece = 1u << 16;                              // 65 536 lines: 2.5 MiB of offsets and records
    const uint64_t n_pieces = (n_lines + piece - 1) / piece;
    const size_t part_bytes = (size_t)4 << 20;                    // the load's pinned staging ring (16 MiB buffers), in parts of 4 MiB
    static_assert((size_t)(1u << 16) * (8 + sizeof(snpgpu_line_record)) <= ((size_t)4 << 20), "a piece fits a part");
    snpgpu_stream_pool *pool_ = ctx->pool;
    const uint32_t parts_per = pool_ ? (uint32_t)(pool_->chunk_bytes / part_bytes) : 0;
    const uint32_t parts = pool_ ? (uint32_t)pool_->staging.size() * parts_per : 0;
    if (n_pieces && parts < 2) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "no pinned staging memory for the records");
    const uint32_t T = n_pieces ? (uint32_t)std::min<uint64_t>(std::min<uint32_t>(snpgpu_cpu_threads(64), parts - 1), n_pieces) : 0;
    const uint32_t R = n_pieces ? (uint32_t)std::min<uint64_t>(std::min<uint32_t>(T + 2, parts), n_pieces) : 0;          // parts in flight
    std::vector<void *> pinned(R, nullptr);
    std::vector<hipEvent_t> ev(R, nullptr);
    hipError_t he = hipSuccess;
    for (uint32_t k = 0; k < R && he == hipSuccess; ++k) {
        pinned[k] = (char *)pool_->staging[k / parts_per] + (size_t)(k % parts_per) * part_bytes;
        he = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
    }
    struct Piece { std::vector<char> text; uint64_t rows = 0; bool done = false, bad = false; uint64_t bad_line = 0; };
    std::vector<Piece> out(n_pieces);
    std::mutex mu;
    std::condition_variable cv;
    std::vector<int> landed(n_pieces, 0);                       // 1: its copies were enqueued (the event tells when they are done)
    std::vector<int> buffer_free(R, 1);
    std::atomic<uint64_t> next_piece{0};
    uint64_t written_upto = 0, file_off = header_len;           // (under mu) pieces whose text is in the file
    bool abort_all = he != hipSuccess;
    auto worker = [&]() {
        (void)hipSetDevice(ctx->device);
        for (;;) {
            const uint64_t pi = next_piece.fetch_add(1);
            if (pi >= n_pieces) return;
            const uint32_t k = (uint32_t)(pi % R);
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return landed[pi] || abort_all; }); if (abort_all) return; }
            if (hipEventSynchronize(ev[k]) != hipSuccess) { std::lock_guard<std::mutex> lk(mu); abort_all = true; cv.notify_all(); return; }
            const uint64_t lo = pi * piece, hi = std::min<uint64_t>(n_lines, lo + piece);
            const uint64_t *off = (const uint64_t *)pinned[k];
            const snpgpu_line_record *recs = (const snpgpu_line_record *)((const char *)pinned[k] + 8 * piece);
            Piece &pc = out[pi];
            pc.bad = !snpgpu_line_rows_into(text, al.nbytes, off, recs, lo, lo, hi, wide_index.data(), wide.data(), n_wide, filter_names, preserve_ref_case,
                                              failed_snp_gt, spill.data(), n_spill, only_listed, pc.text, &pc.rows, &pc.bad_line);
            std::unique_lock<std::mutex> lk(mu);
            buffer_free[k] = 1;
            pc.done = true;
            cv.notify_all();
            // the file is written in piece order by whoever finishes the piece that is next in line
            while (written_upto < n_pieces && out[written_upto].done && !abort_all) {
                Piece &w = out[written_upto];
                const uint64_t at = file_off;
                file_off += w.text.size();
                const uint64_t me = written_upto++;
                lk.unlock();
                if (io_ok && !w.bad) {
                    const char *p = w.text.data();
                    size_t left = w.text.size();
                    uint64_t pos = at;
                    while (left) {
                        const ssize_t wr = pwrite(vfd, p, left, (off_t)pos);
                        if (wr < 0) { if (errno == EINTR) continue; io_ok = false; break; }
                        p += wr; left -= (size_t)wr; pos += (uint64_t)wr;
                    }
                }
                std::vector<char>().swap(out[me].text);
                lk.lock();
            }
        }
    };
    std::vector<std::thread> pool;
    if (!abort_all) for (uint32_t t = 0; t < T; ++t) pool.emplace_back(worker);
    if (io_ok && header_len) {
        size_t left = header_len; const char *p = header; uint64_t pos = 0;
        while (left) { const ssize_t wr = pwrite(vfd, p, left, (off_t)pos); if (wr < 0) { if (errno == EINTR) continue; io_ok = false; break; } p += wr; left -= (size_t)wr; pos += (uint64_t)wr; }
    }
    for (uint64_t pi = 0; pi < n_pieces && !abort_all; ++pi) {
        const uint32_t k = (uint32_t)(pi % R);
        { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return buffer_free[k] || abort_all; }); if (abort_all) break; buffer_free[k] = 0; }
        const uint64_t lo = pi * piece, hi = std::min<uint64_t>(n_lines, lo + piece);
        he = hipMemcpyAsync(pinned[k], al.d_off + lo, 8 * (hi - lo), hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync((char *)pinned[k] + 8 * piece, al.d_recs + lo, sizeof(snpgpu_line_record) * (hi - lo), hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipEventRecord(ev[k], st);
        std::lock_guard<std::mutex> lk(mu);
        if (he != hipSuccess) abort_all = true; else landed[pi] = 1;
        cv.notify_all();
    }
    { std::lock_guard<std::mutex> lk(mu); cv.notify_all(); }
    for (auto &t : pool) t.join();
    (void)hipStreamSynchronize(st);
    for (uint32_t k = 0; k < R; ++k) if (ev[k]) (void)hipEventDestroy(ev[k]);
    if (text) { munmap((void *)text, al.nbytes); close(pfd); }
    uint64_t rows = 0, bad_line = ~0ull;
    for (auto &pc : out) { rows += pc.rows; if (pc.bad && bad_line == ~0ull) bad_line = pc.bad_line; }
    if (vfd >= 0) {
        if (io_ok && ftruncate(vfd, (off_t)file_off) != 0) io_ok = false;
        if (close(vfd) != 0) io_ok = false;
    }
    if (he != hipSuccess || abort_all) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "reading the records of %s back failed: %s", pileup_path, hipGetErrorString(he));
    if (bad_line != ~0ull) return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "line %llu of %s has more symbols than a record keeps and no spill record", (unsigned long long)bad_line, pileup_path);
    if (!io_ok) return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot write %s", vcf_path);
    *out_n_rows = rows;
    return SNPGPU_OK;
}

}  // extern "C"

namespace {

// Phase-1 site calling over a pileup that is in device memory: one pass over the text (line starts + select) and a walk over the
// few candidate lines on the device (varscan.hip), records back in file order.  Synchronous.
int varscan_resident(snpgpu_ctx *ctx, const uint8_t *d_file, uint64_t nbytes, const char *what, const snpgpu_varscan_params *params,
                     uint32_t capacity, snpgpu_varscan_site *out_sites, uint32_t *out_n_sites, uint64_t *out_status) {
    hipStream_t st = ctx->stream;
    *out_n_sites = 0;
    out_status[0] = ~0ull; out_status[1] = 0;
    if (nbytes == 0) return SNPGPU_OK;
    size_t o = 0;
    const size_t o_ctl = o; o += 256;                          // [0] u64 status, then the kernels' eight control words
    const size_t o_rec = o; o += up(sizeof(snpgpu_varscan_site) * (size_t)capacity, 256);
    const size_t o_var = o; o += up(snpgpu_varscan_scratch_bytes(nbytes), 256);
    void *scr = nullptr;
    int rc = snpgpu_scratch(ctx, o + 256, &scr);
    if (rc) return rc;
    char *b = (char *)scr;
    uint64_t h_ctl[5] = {~0ull, 0, 0, 0, 0};                    // status; records found + candidates; long candidates + spare; lines; spare
    HIP_TRY(ctx, hipMemcpyAsync(b + o_ctl, h_ctl, sizeof h_ctl, hipMemcpyHostToDevice, st));
    rc = snpgpu_enqueue_varscan(ctx, d_file, nbytes, params, (snpgpu_varscan_site *)(b + o_rec), capacity, (uint32_t *)(b + o_ctl + 8), (uint64_t *)(b + o_ctl),
                                b + o_var);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(h_ctl, b + o_ctl, sizeof h_ctl, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
#ifdef SNPGPU_TUNING
    if (getenv("SNPGPU_VARSCAN_DEBUG"))
        fprintf(stderr, "varscan: %llu lines, %u candidates on the global list\n", (unsigned long long)h_ctl[3], (uint32_t)(h_ctl[1] >> 32));
#endif
    out_status[0] = h_ctl[0];
    out_status[1] = h_ctl[3];
    const uint32_t found = (uint32_t)h_ctl[1];
    *out_n_sites = found;
    if (h_ctl[0] != ~0ull)
        return snpgpu_set_error(ctx, SNPGPU_E_PILEUP, "malformed pileup line at byte %llu of %s", (unsigned long long)h_ctl[0], what);
    const uint32_t got = found < capacity ? found : capacity;
    if (got) {
        HIP_TRY(ctx, hipMemcpyAsync(out_sites, b + o_rec, sizeof(snpgpu_varscan_site) * (size_t)got, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (found <= capacity)
            std::sort(out_sites, out_sites + got, [](const snpgpu_varscan_site &x, const snpgpu_varscan_site &y) {
                return x.line_off != y.line_off ? x.line_off < y.line_off : x.alt_base < y.alt_base;
            });
    }
    return SNPGPU_OK;
}

// The same for many resident pileups at once: ONE scan launch over all of them (varscan.hip), one copy of the control words back,
// then the records of every file.  Synchronous.  out_sites [n_files][capacity], out_n_sites [n_files], out_status [n_files][2],
// out_rc [n_files].
int varscan_resident_batch(snpgpu_ctx *ctx, const void *const *d_pileups, const uint64_t *nbytes, uint32_t n_files, const snpgpu_varscan_params *params,
                           uint32_t capacity, snpgpu_varscan_site *out_sites, uint32_t *out_n_sites, uint64_t *out_status, int32_t *out_rc) {
    hipStream_t st = ctx->stream;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_files; ++i) {
        if (nbytes[i] && !d_pileups[i]) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null pileup %u", i);
        total += nbytes[i];
        out_n_sites[i] = 0; out_status[2 * i] = ~0ull; out_status[2 * i + 1] = 0; out_rc[i] = SNPGPU_OK;
    }
    size_t o = 0;
    const size_t o_ctl = o; o += up(40 * (size_t)n_files, 256);                      // per file: u64 status, eight control words
    const size_t o_rec = o; o += up(sizeof(snpgpu_varscan_site) * (size_t)capacity * n_files, 256);
    const size_t o_var = o; o += up(snpgpu_varscan_batch_scratch_bytes(total, n_files), 256);
    void *scr = nullptr;
    int rc = snpgpu_scratch(ctx, o + 256, &scr);
    if (rc) return rc;
    char *b = (char *)scr;
    // the status words first (n_files u64), then the control words (n_files x 8 u32)
    std::vector<uint64_t> h_ctl(5 * (size_t)n_files, 0);
    for (uint32_t i = 0; i < n_files; ++i) h_ctl[i] = ~0ull;
    std::vector<char> h_table(snpgpu_varscan_table_bytes(n_files));
    HIP_TRY(ctx, hipMemcpyAsync(b + o_ctl, h_ctl.data(), 40 * (size_t)n_files, hipMemcpyHostToDevice, st));
    rc = snpgpu_enqueue_varscan_batch(ctx, (const uint8_t *const *)d_pileups, nbytes, n_files, params, (snpgpu_varscan_site *)(b + o_rec), capacity,
                                      (uint32_t *)(b + o_ctl + 8 * (size_t)n_files), (uint64_t *)(b + o_ctl), b + o_var, h_table.data());
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    HIP_TRY(ctx, hipMemcpyAsync(h_ctl.data(), b + o_ctl, 40 * (size_t)n_files, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                   // (h_table and h_ctl have been read by then)
    const uint32_t *words = (const uint32_t *)(h_ctl.data() + n_files);
    for (uint32_t i = 0; i < n_files; ++i) {
        const uint32_t *w = words + 8 * (size_t)i;
        uint64_t lines;
        memcpy(&lines, w + 4, 8);
        out_status[2 * i] = h_ctl[i];
        out_status[2 * i + 1] = lines;
        out_n_sites[i] = w[0];
        if (h_ctl[i] != ~0ull) { out_rc[i] = SNPGPU_E_PILEUP; continue; }
        const uint32_t got = w[0] < capacity ? w[0] : capacity;
        if (got) HIP_TRY(ctx, hipMemcpyAsync(out_sites + (size_t)i * capacity, b + o_rec + sizeof(snpgpu_varscan_site) * (size_t)capacity * i,
                                             sizeof(snpgpu_varscan_site) * (size_t)got, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n_files; ++i) {
        if (out_rc[i] != SNPGPU_OK || out_n_sites[i] > capacity) continue;           // (more records than the array holds: the caller repeats that file alone)
        snpgpu_varscan_site *dst = out_sites + (size_t)i * capacity;
        std::sort(dst, dst + out_n_sites[i], [](const snpgpu_varscan_site &x, const snpgpu_varscan_site &y) {
            return x.line_off != y.line_off ? x.line_off < y.line_off : x.alt_base < y.alt_base;
        });
    }
    return SNPGPU_OK;
}

// Device memory for the files of one ingest call that are to stay resident: whole files, 256-byte aligned, bump-allocated out
// of blocks of at most `block_cap` bytes (a block is allocated right before the first copy into it).  Files are placed in
// order while the budget lasts; from the first one that does not fit on, they stay non-resident.
struct Placement { uint32_t block; uint64_t off; };
const uint64_t PILEUP_BLOCK_CAP = 8ull << 30;
const uint64_t PILEUP_TAIL_PAD = SNPGPU_SCAN_TILE + 512;       // the scan reads whole tiles (+ halo) past a file's last byte

// What the readers and the issuing thread share when pieces may be copied in ANY order (resident files: every piece has its
// own place in device memory, so nobody has to wait for the slowest read — with the in-order ring one slow pread stalls the
// copy engine and, a few pieces later, every other reader).
struct AnyOrder {
    std::mutex mu;
    std::condition_variable cv_free, cv_ready;
    std::vector<uint32_t> free_bufs;
    struct Ready { uint64_t job; int32_t buf; int err; };
    std::deque<Ready> ready;
    bool abort = false;
    std::atomic<uint64_t> next{0};
    uint64_t n_jobs = 0;
    std::atomic<uint64_t> ns_reading{0}, ns_waiting{0};
    Opener *opener = nullptr;
    std::vector<std::thread> readers;
};

void reader_any_order(snpgpu_ctx *ctx, AnyOrder *sh, const std::vector<Job> *jobs, std::vector<Source> *src) {
    snpgpu_stream_pool *p = ctx->pool;
    if (p->have_near_cpus) (void)sched_setaffinity(0, sizeof p->near_cpus, &p->near_cpus);
    for (;;) {
        const uint64_t j = sh->next.fetch_add(1);
        if (j >= sh->n_jobs) return;
        const Job &jb = (*jobs)[j];
        int32_t buf = -1;
        int err = 0;
        if (jb.len) {
            const double t_w = now_s();
            if (sh->opener) sh->opener->wait(jb.file);
            {
                std::unique_lock<std::mutex> lk(sh->mu);
                sh->cv_free.wait(lk, [&] { return sh->abort || !sh->free_bufs.empty(); });
                if (sh->abort) return;
                buf = (int32_t)sh->free_bufs.back();
                sh->free_bufs.pop_back();
            }
            const double t_r = now_s();
            err = read_piece((*src)[jb.file], jb, (uint8_t *)p->staging[buf]);
            sh->ns_waiting.fetch_add((uint64_t)((t_r - t_w) * 1e9));
            sh->ns_reading.fetch_add((uint64_t)((now_s() - t_r) * 1e9));
        }
        if (sh->opener) sh->opener->done_reading(jb.file);
        {
            std::lock_guard<std::mutex> lk(sh->mu);
            sh->ready.push_back(AnyOrder::Ready{j, buf, err});
        }
        sh->cv_ready.notify_one();
    }
}

// Phase-1 site calling over many pileup files: the readers run ahead across file boundaries, and a file's kernels and result
// copy run on the compute stream while the next files are being read and copied.  Without a store the files alternate between
// two device slots and their pieces are copied in file order; with one, files go to resident memory while the store's budget
// lasts (entry store->files[first + f]), their pieces copied in whatever order the reads finish, and only the files past the
// budget use the slots.  params == nullptr: no site calling, the files are only made resident.  out_done (nullable): out_done[f]
// becomes 1 when the outputs of file f are final, so that another thread can start on them while the call is still running.
int varscan_stream(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, const snpgpu_varscan_params *params, uint32_t capacity,
                   snpgpu_varscan_site *out_sites, uint32_t *out_n_sites, uint64_t *out_status, int32_t *out_rc, snpgpu_pileups *store,
                   int32_t *out_done) {
    HIP_TRY(ctx, snpgpu_enter(ctx));
    const double t_enter = now_s();
    // pieces of 32 MiB: 53-54 GB/s of files into resident memory where 16 MiB pieces give 50-52 (fewer, larger preads and copies;
    // 64 MiB: 46 — the pipeline of 12 staging buffers gets too coarse); tools/pipeline_time.py with SNPGPU_INGEST_CHUNK_MIB
    size_t chunk = (size_t)32 << 20;
#ifdef SNPGPU_TUNING                                            // development builds only (tools/)
    if (const char *e = getenv("SNPGPU_INGEST_CHUNK_MIB")) if (atoi(e) > 0) chunk = (size_t)atoi(e) << 20;
#endif
    std::vector<Source> src(n_files);
    uint64_t max_slot_size = 0;
    const size_t first = store ? store->files.size() : 0;
    if (store) store->files.resize(first + n_files);
    std::vector<Placement> place(n_files, Placement{~0u, 0});
    std::vector<uint64_t> block_bytes;                          // blocks of this call
    uint32_t n_prefix = 0;                                      // files [0, n_prefix) are resident (or have nothing to copy)
    bool budget_left = store != nullptr;
    for (uint32_t f = 0; f < n_files; ++f) {
        Source &s = src[f];
        s.path = paths[f];
        size_source(s);                                         // (the file itself is opened later, by the opener thread)
        bool resident = false;
        if (budget_left && s.rc == SNPGPU_OK) {
            const uint64_t need = up(s.size + 1, 256);
            if (store->used + need + PILEUP_TAIL_PAD <= store->budget) {
                // (the first blocks are small — 1, 2, 4 GiB, then 8 — so that the first copy does not wait for a large allocation)
                const uint64_t cap_now = block_bytes.size() <= 3 ? (PILEUP_BLOCK_CAP >> (4 - (block_bytes.size() ? block_bytes.size() : 1))) : PILEUP_BLOCK_CAP;
                if (block_bytes.empty() || block_bytes.back() + need + PILEUP_TAIL_PAD > cap_now) { block_bytes.push_back(0); store->used += PILEUP_TAIL_PAD; }
                place[f] = Placement{(uint32_t)(block_bytes.size() - 1), block_bytes.back()};
                block_bytes.back() += need;
                store->used += need;
                resident = true;
            } else {
                budget_left = false;
            }
        }
        if (store && n_prefix == f && (resident || s.rc != SNPGPU_OK || s.size == 0)) n_prefix = f + 1;
        if (store) {
            store->files[first + f].nbytes = s.size;
            store->files[first + f].resident = resident;
            store->file_bytes += s.size;
        }
        if (!resident && s.size > max_slot_size) max_slot_size = s.size;
        out_n_sites[f] = 0;
        out_status[2 * f] = ~0ull; out_status[2 * f + 1] = 0;
        if (out_done) out_done[f] = 0;
    }
    for (auto &b : block_bytes) b += PILEUP_TAIL_PAD;
    [[maybe_unused]] const double t_opened = now_s();
    std::vector<uint8_t *> block_ptr(block_bytes.size(), nullptr);
    std::vector<uint8_t> block_seen(block_bytes.size(), 0);     // the issuing thread has waited for the block's allocation
    std::vector<Job> jobs;
    std::vector<uint32_t> chunks_left(n_files, 0);
    uint64_t JA = 0;                                            // jobs [0, JA): files of the prefix; [JA, J): the rest, in file order
    for (uint32_t f = 0; f < n_files; ++f) {
        const uint64_t n = src[f].size;
        if (f == n_prefix) JA = jobs.size();
        if (n == 0) { jobs.push_back(Job{f, 0, 0, true, true, 0}); chunks_left[f] = 1; continue; }
        for (uint64_t off = 0, c = 0; off < n; ++c) {
            const uint64_t want = f == 0 ? ramp_piece(c, chunk) : chunk, len = n - off < want ? n - off : want;
            jobs.push_back(Job{f, off, len, c == 0, off + len >= n, (uint32_t)c});
            ++chunks_left[f];
            off += len;
        }
    }
    const uint64_t J = jobs.size();
    if (n_prefix == n_files) JA = J;
    uint32_t n_readers = snpgpu_reader_threads();
    uint32_t extra_staging = 4;
#ifdef SNPGPU_TUNING                                            // development builds only (tools/)
    if (const char *e = getenv("SNPGPU_INGEST_READERS")) if (atoi(e) > 0) n_readers = (uint32_t)atoi(e);
    if (const char *e = getenv("SNPGPU_INGEST_EXTRA_STAGING")) if (atoi(e) >= 0) extra_staging = (uint32_t)atoi(e);
#endif
    uint32_t n_staging;
    ring_sizes(J, n_readers, extra_staging, &n_readers, &n_staging);
    if (store) store->n_readers = n_readers;
    const size_t r_rec = 256;                                  // result block: [0] u64 status, [8] u32 records found, [48] u32 lines; records at 256
    const size_t result_bytes = r_rec + sizeof(snpgpu_varscan_site) * (size_t)capacity + 256;
    Opener opener;
    auto close_all = [&]() { opener.finish(); for (auto &s2 : src) if (s2.fd >= 0) { close(s2.fd); s2.fd = -1; } };
    opener.start(&src, chunks_left);                            // (the first files open while the staging memory is being pinned)
    const uint32_t n_slots = n_files > 1 ? 2 : 1;              // result blocks / scratch halves (/ device slots) alternate between files
    const bool any_slot = n_prefix < n_files;
    int rc = pool_ensure(ctx, chunk, n_staging, any_slot ? n_slots : 0, any_slot ? up(max_slot_size + SNPGPU_SCAN_TILE + 256, 4096) : 0,
                         result_bytes, 256, n_slots);
    if (rc) { close_all(); return rc; }
    snpgpu_stream_pool *p = ctx->pool;                          // (both passes use its first n_staging staging buffers)
    hipStream_t st = ctx->stream;
    [[maybe_unused]] const double t_pool = now_s();
    {
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) { close_all(); return snpgpu_set_error(ctx, SNPGPU_E_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e)); }
    }
#ifdef SNPGPU_TUNING
    if (getenv("SNPGPU_VARSCAN_DEBUG"))
        fprintf(stderr, "ingest prepare: files sized and placed %.4f s, staging pool %.4f s, stream idle %.4f s\n", t_opened - t_enter,
                t_pool - t_opened, now_s() - t_pool);
#endif
    // Files are post-processed in the order in which they become complete ("sequence numbers"); result blocks, scratch halves
    // and device slots alternate by sequence number.
    std::vector<int64_t> seq_of(n_files, -1);
    std::vector<uint32_t> file_of;
    file_of.reserve(n_files);
    auto dest = [&](uint32_t f) -> uint8_t * {
        if (place[f].block == ~0u) return (uint8_t *)p->slot[(uint32_t)seq_of[f] % n_slots];
        return block_ptr[place[f].block] + place[f].off;
    };
    std::vector<uint8_t> has_result(n_files, 0), completed(n_files, 0);   // by sequence number
    const double t_begin = now_s();
    double t_alloc = 0, t_read_wait = 0, t_dev_wait = 0;
    uint64_t ns_reading = 0, ns_waiting = 0;
    auto publish = [&](uint32_t f) { if (out_done) __atomic_store_n(&out_done[f], 1, __ATOMIC_RELEASE); };
    auto harvest = [&](uint32_t c) -> int {                     // results of the c-th completed file: pinned block -> the caller's arrays
        const uint32_t f = file_of[c];
        if (!has_result[c]) { out_rc[f] = src[f].rc; publish(f); return SNPGPU_OK; }
        const uint32_t slot = c % n_slots;
        const double tw = now_s();
        hipError_t e = hipEventSynchronize(p->ev_done[slot]);
        t_dev_wait += now_s() - tw;
        if (e != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "waiting for the results of pileup %u failed: %s", f, hipGetErrorString(e));
        const char *r = (const char *)p->result[slot];
        uint64_t status;
        uint32_t found;
        memcpy(&status, r, 8);
        memcpy(&found, r + 8, 4);
        memcpy(&out_status[2 * f + 1], r + 24, 8);              // the file's line count
        out_status[2 * f] = status;
        out_n_sites[f] = found;
        if (status != ~0ull) { if (src[f].rc == SNPGPU_OK) src[f].rc = SNPGPU_E_PILEUP; out_rc[f] = src[f].rc; publish(f); return SNPGPU_OK; }
        const uint32_t got = found < capacity ? found : capacity;
        snpgpu_varscan_site *dst = out_sites + (size_t)f * capacity;
        if (got) memcpy(dst, r + r_rec, sizeof(snpgpu_varscan_site) * (size_t)got);
        if (found <= capacity)
            std::sort(dst, dst + got, [](const snpgpu_varscan_site &x, const snpgpu_varscan_site &y) {
                return x.line_off != y.line_off ? x.line_off < y.line_off : x.alt_base < y.alt_base;
            });
        out_rc[f] = src[f].rc;
        publish(f);
        return SNPGPU_OK;
    };
    // The work on a complete file: one pass over its text, the walk over the candidates, results into the slot's pinned block.
    // Nothing here waits for the device (round 3 needed the file's line count on the host between two halves of this).
#define VS_RET(expr)                                                                                                \
    do {                                                                                                            \
        hipError_t e_ = (expr);                                                                                     \
        if (e_ != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
    auto post = [&](uint32_t c) -> int {
        const uint32_t f = file_of[c], slot = c % n_slots;
        const uint64_t nbytes = src[f].size;
        const uint8_t *d_file = dest(f);
        char *res = (char *)p->result[slot];
        size_t o = 0;
        const size_t o_ctl = o; o += 256;
        const size_t o_rec = o; o += up(sizeof(snpgpu_varscan_site) * (size_t)capacity, 256) + 256;
        const size_t o_var = o; o += up(snpgpu_varscan_scratch_bytes(nbytes), 256);
        void *scr = nullptr;
        int r = snpgpu_scratch(ctx, 2 * o + 512, &scr);         // may move the scratch (it waits for the compute stream first)
        if (r) return r;
        const size_t half = ctx->scratch_bytes / 2 / 256 * 256;
        char *b = (char *)scr + half * slot;
        uint64_t h_ctl[5] = {~0ull, 0, 0, 0, 0};                // status; records found + candidates; long candidates + spare; lines; spare
        memcpy(res + 64, h_ctl, sizeof h_ctl);                  // (a pinned source that stays valid until the copy has run)
        VS_RET(hipMemcpyAsync(b + o_ctl, res + 64, sizeof h_ctl, hipMemcpyHostToDevice, st));
        r = snpgpu_enqueue_varscan(ctx, d_file, nbytes, params, (snpgpu_varscan_site *)(b + o_rec), capacity, (uint32_t *)(b + o_ctl + 8), (uint64_t *)(b + o_ctl),
                                   b + o_var);
        if (r) return r;
        VS_RET(hipMemcpyAsync(res, b + o_ctl, 32, hipMemcpyDeviceToHost, st));
        if (capacity) VS_RET(hipMemcpyAsync(res + r_rec, b + o_rec, sizeof(snpgpu_varscan_site) * (size_t)capacity, hipMemcpyDeviceToHost, st));
        VS_RET(hipEventRecord(p->ev_done[slot], st));
        has_result[c] = 1;
        return SNPGPU_OK;
    };
#undef VS_RET
    uint32_t harvested = 0;                                     // sequence numbers [0, harvested) have been copied out
    // file f is complete (every piece issued): give it its sequence number (unless it has one) and start its post-processing
    auto file_complete = [&](uint32_t f) -> int {
        if (seq_of[f] < 0) { seq_of[f] = (int64_t)file_of.size(); file_of.push_back(f); }
        const uint32_t c = (uint32_t)seq_of[f];
        completed[c] = 1;
        if (!params || src[f].rc != SNPGPU_OK || src[f].size == 0) return SNPGPU_OK;
        int r = SNPGPU_OK;
        while (!r && harvested + n_slots <= c) r = harvest(harvested++);           // its result block and scratch half are free then
        if (!r) r = post(c);
        return r;
    };
    // what can be done without waiting: hand out results that are ready
    auto opportunistic = [&]() -> int {
        int r = SNPGPU_OK;
        while (!r && harvested < file_of.size() && completed[harvested] &&
               (!has_result[harvested] || hipEventQuery(p->ev_done[harvested % n_slots]) != hipErrorNotReady))
            r = harvest(harvested++);
        return r;
    };
    {
        // ---- pass A: the resident prefix, pieces copied in the order in which their reads finish -----------------------------
        if (JA) {
            AnyOrder sh;
            sh.n_jobs = JA;
            sh.opener = &opener;
            rc = start_readers(ctx, sh, sh.cv_free, JA, n_readers < JA ? n_readers : (uint32_t)JA,
                               [&] { for (uint32_t i = 0; i < n_staging; ++i) sh.free_bufs.push_back(i); }, reader_any_order, &jobs, &src);
            if (rc) goto done;
            // The blocks are allocated by a helper thread, in the order in which they will be needed, while this thread copies
            // into the ones that exist: an allocation from the driver costs ~15 ms per GiB (and many times that for memory that
            // was freed a moment ago), about as long as the copy into it, but it does not hold up copies issued by another thread
            // (tools/probe/alloc_dirty_probe.cpp).
            std::mutex alloc_mu;
            std::condition_variable alloc_cv;
            std::vector<hipError_t> alloc_err(block_bytes.size(), hipSuccess);
            std::vector<uint8_t> alloc_done(block_bytes.size(), 0);
            std::atomic<bool> alloc_stop{false};
            double alloc_thread_seconds = 0;
            auto allocate_all = [&] {
                (void)hipSetDevice(ctx->device);
                for (size_t b = 0; b < block_bytes.size() && !alloc_stop.load(); ++b) {
                    void *d = nullptr;
                    const double ta = now_s();
                    const hipError_t e = hipMalloc(&d, block_bytes[b]);
                    alloc_thread_seconds += now_s() - ta;
                    {
                        std::lock_guard<std::mutex> lk(alloc_mu);
                        block_ptr[b] = e == hipSuccess ? (uint8_t *)d : nullptr;
                        alloc_err[b] = e;
                        alloc_done[b] = 1;
                    }
                    alloc_cv.notify_all();
                    if (e != hipSuccess) break;
                }
            };
            std::thread allocator;
            try { allocator = std::thread(allocate_all); } catch (const std::exception &) { allocate_all(); }      // no thread to be had: up front, here
            std::deque<uint32_t> inflight;                      // staging buffers whose copies are on their way, in issue order per stream pair
            uint64_t issued = 0;
            int rcA = SNPGPU_OK;
            while (issued < JA && !rcA) {
                // staging buffers whose copy has finished go back to the readers
                bool freed = false;
                while (!inflight.empty() && hipEventQuery(p->ev_copy[inflight.front()]) != hipErrorNotReady) {
                    std::lock_guard<std::mutex> lk(sh.mu);
                    sh.free_bufs.push_back(inflight.front());
                    inflight.pop_front();
                    freed = true;
                }
                if (freed) sh.cv_free.notify_all();
                rcA = opportunistic();
                if (rcA) break;
                AnyOrder::Ready rd{0, -1, 0};
                bool have = false;
                {
                    const double tr = now_s();
                    std::unique_lock<std::mutex> lk(sh.mu);
                    if (sh.ready.empty())
                        sh.cv_ready.wait_for(lk, std::chrono::microseconds(inflight.empty() ? 2000 : 20), [&] { return !sh.ready.empty(); });
                    if (!sh.ready.empty()) { rd = sh.ready.front(); sh.ready.pop_front(); have = true; }
                    lk.unlock();
                    t_read_wait += now_s() - tr;
                }
                if (!have) continue;
                const Job &jb = jobs[rd.job];
                const uint32_t f = jb.file;
                Source &s = src[f];
                if (rd.err && s.rc == SNPGPU_OK) s.rc = SNPGPU_E_IO;
                if (place[f].block != ~0u && !block_seen[place[f].block]) {
                    const uint32_t b = place[f].block;
                    const double ta = now_s();
                    hipError_t e;
                    {
                        std::unique_lock<std::mutex> lk(alloc_mu);
                        alloc_cv.wait(lk, [&] { return alloc_done[b] != 0 || (b > 0 && alloc_done[b - 1] && alloc_err[b - 1] != hipSuccess); });
                        e = alloc_done[b] ? alloc_err[b] : hipErrorOutOfMemory;
                    }
                    t_alloc += now_s() - ta;
                    if (e != hipSuccess) {
                        rcA = snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "hipMalloc(%llu) for resident pileups failed: %s", (unsigned long long)block_bytes[b], hipGetErrorString(e));
                        break;
                    }
                    block_seen[b] = 1;
                }
                if (place[f].block != ~0u) store->files[first + f].d = dest(f);
                if (jb.len) {
                    hipStream_t cs = (issued & 1) ? p->copy_stream2 : p->copy_stream;
                    hipError_t e = hipMemcpyAsync(dest(f) + jb.off, p->staging[rd.buf], jb.len, hipMemcpyHostToDevice, cs);
                    if (e == hipSuccess) e = hipEventRecord(p->ev_copy[rd.buf], cs);
                    if (e == hipSuccess) e = hipStreamWaitEvent(st, p->ev_copy[rd.buf], 0);
                    if (e != hipSuccess) { rcA = snpgpu_set_error(ctx, SNPGPU_E_HIP, "copying a piece of %s failed: %s", s.path, hipGetErrorString(e)); break; }
                    store->h2d_bytes += jb.len;
                    // (the two copy streams finish their copies in their own order: a buffer is retired when the one at the head of
                    // the queue is — at most one copy later than it could be)
                    inflight.push_back((uint32_t)rd.buf);
                }
                ++issued;
                if (--chunks_left[f] == 0) rcA = file_complete(f);
            }
            stop_readers(sh, sh.cv_free, JA, rcA != SNPGPU_OK);
            if (rcA) alloc_stop.store(true);
            if (allocator.joinable()) allocator.join();
#ifdef SNPGPU_TUNING
            if (getenv("SNPGPU_VARSCAN_DEBUG")) fprintf(stderr, "ingest: the allocator thread spent %.3f s in hipMalloc (%zu blocks)\n", alloc_thread_seconds, block_bytes.size());
#endif
            for (size_t b = 0; b < block_ptr.size(); ++b) if (block_ptr[b]) store->blocks.push_back(block_ptr[b]);      // the store owns them, used or not
            ns_reading += sh.ns_reading.load();
            ns_waiting += sh.ns_waiting.load();
            if (rcA) { rc = rcA; goto done; }
            // every staging buffer is free again before the in-order ring of pass B uses them
            if (JA < J) { STREAM_TRY(hipStreamSynchronize(p->copy_stream)); STREAM_TRY(hipStreamSynchronize(p->copy_stream2)); }
        }
        // ---- pass B: files that go through the device slots, pieces in file order -------------------------------------------
        if (JA < J) {
            Ring ring;
            rc = ring.start(ctx, &jobs, &src, JA, J - JA, n_staging, n_readers, &opener);
            if (rc) goto done;
            int rcB = SNPGPU_OK;
            for (uint64_t j = JA; j < J && !rcB; ++j) {
                const Job &jb = jobs[j];
                const uint32_t f = jb.file;
                Source &s = src[f];
                rcB = opportunistic();
                if (rcB) break;
                if (jb.first) {                                 // a sequence number now: its slot is where the pieces go
                    seq_of[f] = (int64_t)file_of.size();
                    file_of.push_back(f);
                    const uint32_t c = (uint32_t)seq_of[f];
                    while (!rcB && harvested + n_slots <= c) rcB = harvest(harvested++);
                    if (rcB) break;
                }
                uint8_t *d_file = dest(f);
                const double tr = now_s();
                if (ring.wait(j) && s.rc == SNPGPU_OK) s.rc = SNPGPU_E_IO;
                t_read_wait += now_s() - tr;
                hipStream_t cs = ring.copy_stream(j);
                hipError_t e = hipSuccess;
                if (jb.len) e = hipMemcpyAsync(d_file + jb.off, ring.staging(j), jb.len, hipMemcpyHostToDevice, cs);
                if (store) store->h2d_bytes += jb.len;
                if (e == hipSuccess) e = hipEventRecord(ring.copy_event(j), cs);
                if (e == hipSuccess) e = hipStreamWaitEvent(st, ring.copy_event(j), 0);
                if (e != hipSuccess) { rcB = snpgpu_set_error(ctx, SNPGPU_E_HIP, "copying a piece of %s failed: %s", s.path, hipGetErrorString(e)); break; }
                if (jb.last) rcB = file_complete(f);
            }
            ring.stop(rcB != SNPGPU_OK);
            ns_reading += ring.ns_reading.load();
            ns_waiting += ring.ns_waiting.load();
            if (rcB) { rc = rcB; goto done; }
        }
        while (harvested < file_of.size()) { rc = harvest(harvested++); if (rc) goto done; }
    }
done:
    {   // every copy has landed before the caller looks at resident memory (or reuses a slot)
        hipError_t e1 = hipStreamSynchronize(p->copy_stream), e2 = hipStreamSynchronize(p->copy_stream2);
        if (rc) (void)hipStreamSynchronize(st);
        if (!rc && (e1 != hipSuccess || e2 != hipSuccess)) rc = snpgpu_set_error(ctx, SNPGPU_E_HIP, "pileup copies failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    }
    close_all();
    if (store) {
        store->seconds += now_s() - t_enter;
        store->seconds_preparing += t_begin - t_enter;
        store->seconds_allocating += t_alloc;
        store->seconds_waiting_for_readers += t_read_wait;
        store->seconds_waiting_for_device += t_dev_wait;
        store->reader_seconds_reading += ns_reading * 1e-9;
        store->reader_seconds_waiting += ns_waiting * 1e-9;
    }
    for (uint32_t f = 0; f < n_files; ++f) {
        out_rc[f] = src[f].rc;
        if (store && (src[f].rc == SNPGPU_E_IO || (place[f].block != ~0u && !block_ptr[place[f].block])))
            store->files[first + f].resident = false;                                       // its bytes are void / never arrived
        if (rc && out_done) __atomic_store_n(&out_done[f], 1, __ATOMIC_RELEASE);            // nobody waits for a call that failed
    }
    return rc;
}

}  // namespace

extern "C" {

int snpgpu_varscan_file(snpgpu_ctx *ctx, const char *path, const snpgpu_varscan_params *params, uint32_t capacity,
                        snpgpu_varscan_site *out_sites, uint32_t *out_n_sites, uint64_t *out_status) {
    if (!ctx || !path || !params || !out_n_sites || !out_status) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (capacity && !out_sites) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null output");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    uint8_t *d_file = nullptr;
    uint64_t nbytes = 0;
    int rc = load_raw(ctx, path, 1, 0, &d_file, &nbytes);     // (plain text only: the rows of var.flt.vcf are formatted from the file on the host)
    if (rc) return rc;
    return varscan_resident(ctx, d_file, nbytes, path, params, capacity, out_sites, out_n_sites, out_status);
}

// The same over a pileup that is already in device memory (a resident file of snpgpu_pileups, a synthetic one).
int snpgpu_varscan_dev(snpgpu_ctx *ctx, const void *d_pileup, uint64_t nbytes, const snpgpu_varscan_params *params, uint32_t capacity,
                       snpgpu_varscan_site *out_sites, uint32_t *out_n_sites, uint64_t *out_status) {
    if (!ctx || !params || !out_n_sites || !out_status || (nbytes && !d_pileup)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (capacity && !out_sites) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null output");
    HIP_TRY(ctx, snpgpu_enter(ctx));
    return varscan_resident(ctx, (const uint8_t *)d_pileup, nbytes, "the resident pileup", params, capacity, out_sites, out_n_sites, out_status);
}

// Many resident pileups, one launch.
int snpgpu_varscan_batch_dev(snpgpu_ctx *ctx, const void *const *d_pileups, const uint64_t *nbytes, uint32_t n_files, const snpgpu_varscan_params *params,
                             uint32_t capacity, snpgpu_varscan_site *out_sites, uint32_t *out_n_sites, uint64_t *out_status, int32_t *out_rc) {
    if (!ctx || !params || !out_n_sites || !out_status || !out_rc || (n_files && (!d_pileups || !nbytes)) || (capacity && !out_sites))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (!n_files) return SNPGPU_OK;
    HIP_TRY(ctx, snpgpu_enter(ctx));
    return varscan_resident_batch(ctx, d_pileups, nbytes, n_files, params, capacity, out_sites, out_n_sites, out_status, out_rc);
}

int snpgpu_varscan_files(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, const snpgpu_varscan_params *params, uint32_t capacity,
                         snpgpu_varscan_site *out_sites, uint32_t *out_n_sites, uint64_t *out_status, int32_t *out_rc) {
    if (!ctx || !params || !out_n_sites || !out_status || !out_rc || (n_files && !paths) || (capacity && !out_sites))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (!n_files) return SNPGPU_OK;
    return varscan_stream(ctx, paths, n_files, params, capacity, out_sites, out_n_sites, out_status, out_rc, nullptr, nullptr);
}

// ---- resident pileups: the input side of the one-job pipeline -----------------------------------------------------------
int snpgpu_pileups_create(snpgpu_ctx *ctx, uint64_t budget_bytes, snpgpu_pileups **out) {
    if (!ctx || !out) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    *out = nullptr;
    HIP_TRY(ctx, snpgpu_enter(ctx));
    if (!budget_bytes) {                                        // what is free now, less room for the outputs of the later steps
        size_t free_b = 0, total_b = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
        const uint64_t keep = (uint64_t)24 << 30;
        budget_bytes = free_b > keep ? (uint64_t)free_b - keep : 0;
    }
    snpgpu_pileups *s = new snpgpu_pileups();
    s->ctx = ctx;
    s->budget = budget_bytes;
    *out = s;
    return SNPGPU_OK;
}

void snpgpu_pileups_destroy(snpgpu_pileups *s) {
    if (!s) return;
    if (s->ctx) {
        (void)hipSetDevice(s->ctx->device);
        (void)hipStreamSynchronize(s->ctx->stream);
    }
    for (void *d : s->blocks) if (d) (void)hipFree(d);
    delete s;
}

int snpgpu_pileups_ingest(snpgpu_ctx *ctx, snpgpu_pileups *store, const char *const *paths, uint32_t n_files,
                          const snpgpu_varscan_params *params, uint32_t capacity, snpgpu_varscan_site *out_sites, uint32_t *out_n_sites,
                          uint64_t *out_status, int32_t *out_rc, int32_t *out_done) {
    if (!ctx || !store || store->ctx != ctx || !out_n_sites || !out_status || !out_rc || (n_files && !paths) || (params && capacity && !out_sites))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (!n_files) return SNPGPU_OK;
    return varscan_stream(ctx, paths, n_files, params, params ? capacity : 0, out_sites, out_n_sites, out_status, out_rc, store, out_done);
}

uint32_t snpgpu_pileups_count(const snpgpu_pileups *store) { return store ? (uint32_t)store->files.size() : 0; }

int snpgpu_pileups_get(const snpgpu_pileups *store, uint32_t index, void **d_ptr, uint64_t *nbytes) {
    if (!store || index >= store->files.size()) return SNPGPU_E_ARG;
    const snpgpu_pileups::Entry &e = store->files[index];
    if (d_ptr) *d_ptr = e.resident ? (void *)e.d : nullptr;
    if (nbytes) *nbytes = e.nbytes;
    return SNPGPU_OK;
}

int snpgpu_pileups_get_stats(const snpgpu_pileups *store, snpgpu_pileups_stats *out) {
    if (!store || !out) return SNPGPU_E_ARG;
    memset(out, 0, sizeof *out);
    out->h2d_bytes = store->h2d_bytes;
    out->file_bytes = store->file_bytes;
    out->resident_bytes = store->used;
    out->budget_bytes = store->budget;
    out->n_files = (uint32_t)store->files.size();
    for (const auto &e : store->files) if (e.resident) ++out->n_resident;
    out->seconds = store->seconds;
    out->seconds_allocating = store->seconds_allocating;
    out->seconds_waiting_for_readers = store->seconds_waiting_for_readers;
    out->seconds_waiting_for_device = store->seconds_waiting_for_device;
    out->reader_seconds_reading = store->reader_seconds_reading;
    out->reader_seconds_waiting = store->reader_seconds_waiting;
    out->seconds_preparing = store->seconds_preparing;
    out->n_readers = store->n_readers;
    return SNPGPU_OK;
}

}  // extern "C"

// ---- the SNP counts of VCF files (vcf_count.hip) ----------------------------------------------------------------------------
// The files go through the same reader threads, staging ring and copy streams as the pileups, but nothing of a file stays on the
// device: a staging chunk holds a piece of the file behind the SNPGPU_VCF_LOOK bytes in front of it (read again: 4 KiB per 16 MiB),
// is copied into one of a few device buffers and counted by a launch of its own, whose counts are added to the file's result
// words.  All results come back in one copy at the end.
namespace {

// begin(d_extra): enqueue what has to happen before the first piece; piece(d_buf, len, own_from, job): enqueue the work on one piece;
// end(d_extra): enqueue what follows the last piece and wait for it.  extra_bytes of scratch behind the piece buffers are the caller's.
template <class Begin, class Piece, class End>
int vcf_stream(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, size_t extra_bytes, int32_t *out_rc, Begin begin, Piece piece, End end) {
    constexpr uint32_t N_DEV = 3;                               // device buffers a chunk is counted in
    HIP_TRY(ctx, snpgpu_enter(ctx));
    const size_t chunk = (size_t)16 << 20;                      // the staging chunks of the pileup streams: the pinned ring is shared with them
    const uint64_t step = chunk - SNPGPU_VCF_LOOK - 16;         // new bytes per piece: look-back + piece + a final newline fit into a chunk
    std::vector<Source> src;
    std::vector<Job> jobs;
    std::vector<uint32_t> chunks_of;
    try {                                                       // (no exception may leave through the C ABI: no memory is an error code)
        src.resize(n_files);
        chunks_of.resize(n_files);
        for (uint32_t f = 0; f < n_files; ++f) {
            Source &s = src[f];
            s.path = paths[f];
            size_source(s);
            const uint64_t n = s.size;
            const uint32_t nc = n ? (uint32_t)((n + step - 1) / step) : 1;      // an empty file still takes one (empty) job
            chunks_of[f] = nc;
            for (uint32_t c = 0; c < nc; ++c) {
                const uint64_t lo = (uint64_t)c * step, hi = n - lo < step ? n : lo + step, look = c ? SNPGPU_VCF_LOOK : 0;
                jobs.push_back(Job{f, lo - look, hi - lo + look, c == 0, c + 1 == nc, c});
            }
        }
    } catch (const std::exception &) {
        return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "no memory for the job list of %u files", n_files);
    }
    const uint64_t J = jobs.size();
    // everything that has to be undone lives here, and every exit after this point goes through `done`
    Opener opener;
    Ring ring;
    hipEvent_t ev_counted[N_DEV] = {nullptr, nullptr, nullptr};
    snpgpu_stream_pool *p = nullptr;
    uint8_t *d_buf[N_DEV] = {nullptr, nullptr, nullptr};
    void *d_extra = nullptr;
    hipStream_t st = ctx->stream;
    int rc = SNPGPU_OK;
    bool opened = false;

    try { opener.start(&src, chunks_of); } catch (const std::exception &) { rc = snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "no memory for the file opener"); goto done; }
    opened = true;
    {
        uint32_t n_readers, n_staging;
        ring_sizes(J, snpgpu_reader_threads(), 4, &n_readers, &n_staging);
        rc = pool_ensure(ctx, chunk, n_staging, 0, 0, 0, 0);
        if (rc) goto done;
        p = ctx->pool;
        const size_t buf_bytes = chunk + 256, res_bytes = up(extra_bytes, 256);
        void *ws = nullptr;
        rc = snpgpu_scratch(ctx, N_DEV * buf_bytes + res_bytes + 256, &ws);
        if (rc) goto done;
        for (uint32_t i = 0; i < N_DEV; ++i) d_buf[i] = (uint8_t *)ws + i * buf_bytes;
        d_extra = (uint8_t *)ws + N_DEV * buf_bytes;
        STREAM_TRY(hipStreamSynchronize(st));                       // whatever used the scratch before is done
        for (uint32_t i = 0; i < N_DEV; ++i) STREAM_TRY(hipEventCreateWithFlags(&ev_counted[i], hipEventDisableTiming));
        rc = begin(d_extra);
        if (rc) goto done;
        rc = ring.start(ctx, &jobs, &src, 0, J, n_staging, n_readers, &opener);
        if (rc) goto done;
    }
    {
        for (uint64_t j = 0; j < J; ++j) {
            const Job &jb = jobs[j];
            Source &s = src[jb.file];
            if (ring.wait(j) && s.rc == SNPGPU_OK) s.rc = SNPGPU_E_IO;
            uint8_t *h = (uint8_t *)ring.staging(j);
            uint32_t len = (uint32_t)jb.len;
            if (jb.last && len && h[len - 1] != '\n') h[len++] = '\n';      // a last line without a terminator is a line
            const uint32_t b = (uint32_t)(j % N_DEV);
            hipStream_t cs = ring.copy_stream(j);
            if (j >= N_DEV) STREAM_TRY(hipStreamWaitEvent(cs, ev_counted[b], 0));      // the piece that was in this buffer has been counted
            if (len) STREAM_TRY(hipMemcpyAsync(d_buf[b], h, len, hipMemcpyHostToDevice, cs));
            STREAM_TRY(hipEventRecord(ring.copy_event(j), cs));
            STREAM_TRY(hipStreamWaitEvent(st, ring.copy_event(j), 0));
            if (s.rc == SNPGPU_OK && s.size) {
                rc = piece(d_buf[b], len, jb.first ? 0u : (uint32_t)SNPGPU_VCF_LOOK, jb);
                if (rc) goto done;
            }
            STREAM_TRY(hipEventRecord(ev_counted[b], st));
        }
        rc = end(d_extra);
        if (rc) goto done;
    }
done:
    if (opened) {
        ring.stop(rc != SNPGPU_OK);
        if (rc && p) { (void)hipStreamSynchronize(p->copy_stream); (void)hipStreamSynchronize(p->copy_stream2); (void)hipStreamSynchronize(st); }
        opener.finish();
        for (auto &s2 : src) if (s2.fd >= 0) { close(s2.fd); s2.fd = -1; }
    }
    for (hipEvent_t e : ev_counted) if (e) (void)hipEventDestroy(e);
    if (rc) return rc;
    for (uint32_t f = 0; f < n_files; ++f) out_rc[f] = src[f].rc;   // SNPGPU_E_IO: the file could not be opened or read (its results are void)
    return SNPGPU_OK;
}

int vcf_count_stream(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, uint32_t capacity, uint64_t *out_counts, uint64_t *out_unusual_off,
                     uint64_t *out_status, int32_t *out_rc) {
    const size_t res_words = 3 + (size_t)capacity;
    std::vector<uint64_t> h_res;
    try { h_res.assign((size_t)n_files * res_words, 0); } catch (const std::exception &) { return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "no memory for the results"); }
    hipStream_t st = ctx->stream;
    uint64_t *d_res = nullptr;
    const int rc = vcf_stream(ctx, paths, n_files, 8 * res_words * n_files, out_rc,
        [&](void *d_extra) { d_res = (uint64_t *)d_extra; HIP_TRY(ctx, hipMemsetAsync(d_res, 0, 8 * res_words * n_files, st)); return (int)SNPGPU_OK; },
        [&](const uint8_t *d_buf, uint32_t len, uint32_t own_from, const Job &jb) {
            return snpgpu_enqueue_vcf_count(ctx, d_buf, len, own_from, jb.off, d_res + (size_t)jb.file * res_words, capacity);
        },
        [&](void *) {
            HIP_TRY(ctx, hipMemcpyAsync(h_res.data(), d_res, 8 * res_words * n_files, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            return (int)SNPGPU_OK;
        });
    if (rc) return rc;
    for (uint32_t f = 0; f < n_files; ++f) {
        const uint64_t *r = h_res.data() + (size_t)f * res_words;
        uint64_t *cnt = out_counts + 3 * (size_t)f;
        cnt[0] = r[0]; cnt[1] = r[1]; cnt[2] = r[2];
        uint64_t status = r[2] > capacity ? SNPGPU_VCF_MORE_UNUSUAL : 0;
        const uint64_t n_off = r[2] < capacity ? r[2] : capacity;
        for (uint64_t k = 0; k < n_off; ++k) {
            out_unusual_off[(size_t)f * capacity + k] = r[3 + k];
            if (r[3 + k] >> 63) status |= SNPGPU_VCF_LONG_LINE;
        }
        std::sort(out_unusual_off + (size_t)f * capacity, out_unusual_off + (size_t)f * capacity + n_off);
        out_status[f] = status;
    }
    return SNPGPU_OK;
}


// ---- merge_vcfs (vcf_merge.hip) -----------------------------------------------------------------------------------------------
// The header lines and the #CHROM line of a VCF file: read from its start until the first data line.
bool merge_read_head(const char *path, std::vector<std::string> &header, std::string &chrom_line) {
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return false;
    std::string text;
    char block[65536];
    size_t at = 0;
    bool done = false, ok = true;
    while (!done) {
        const ssize_t got = pread(fd, block, sizeof block, (off_t)text.size());
        if (got < 0) { ok = false; break; }
        text.append(block, (size_t)got);
        const bool eof = got == 0;
        for (;;) {
            size_t end = text.find('\n', at);
            if (end == std::string::npos) { if (!eof) break; end = text.size(); if (end == at) { done = true; break; } }
            std::string line = text.substr(at, end - at);
            if (!line.empty() && line.back() == '\r') line.pop_back();
            at = end + 1;
            if (line.empty()) continue;
            if (line[0] != '#') { done = true; break; }
            if (chrom_line.empty()) { if (line.compare(0, 6, "#CHROM") == 0) chrom_line = line; else header.push_back(line); }
            if (at >= text.size() && eof) { done = true; break; }
        }
        if (eof) done = true;
    }
    close(fd);
    return ok;
}

// The line of the file whose first byte is at `off`, or (bit 63) whose terminator is there; *start: its first byte.
bool merge_read_line(int fd, uint64_t off, std::string &line, uint64_t *start) {
    char block[65536];
    line.clear();
    if (off >> 63) {
        uint64_t at = off & ~(1ull << 63);
        std::string rev;
        bool found = false;
        while (at > 0 && !found) {
            const uint64_t lo = at > sizeof block ? at - sizeof block : 0;
            if (pread(fd, block, at - lo, (off_t)lo) != (ssize_t)(at - lo)) return false;
            uint64_t k = at - lo;
            while (k > 0 && block[k - 1] != '\n') --k;
            found = k > 0;
            line.insert(0, block + k, at - lo - k);
            at = lo + k;
        }
        *start = at;
    } else {
        *start = off;
        for (uint64_t at = off;;) {
            const ssize_t got = pread(fd, block, sizeof block, (off_t)at);
            if (got < 0) return false;
            if (got == 0) break;
            const void *nl = memchr(block, '\n', (size_t)got);
            if (nl) { line.append(block, (const char *)nl - block); break; }
            line.append(block, (size_t)got);
            at += (uint64_t)got;
        }
    }
    if (!line.empty() && line.back() == '\r') line.pop_back();
    return true;
}

struct MergeBuffers {                // everything merge_vcf_files allocates on the device, freed on every way out
    std::vector<void *> d;
    ~MergeBuffers() { for (void *p : d) if (p) (void)hipFree(p); }
    void release(void *p) {         // one of them, early
        for (void *&q : d) if (q == p && p) { (void)hipFree(p); q = nullptr; }
    }
    template <class T> hipError_t get(T **out, size_t bytes) {
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes ? bytes : 256);
        if (e == hipSuccess) d.push_back(p);
        *out = (T *)p;
        return e;
    }
};

constexpr uint32_t MERGE_UNUSUAL_CAP = 1u << 16;            // lines outside the kernel's grammar the host takes in one merge

// the headers: the first file's lines, every file's column name, the filter ids the records are held against
struct MergeInput {
    std::vector<std::string> header, names;
    std::string filt;
    std::vector<uint32_t> filt_off;
    uint64_t total_bytes = 0;
};

int merge_read_input(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, snpgpu_merge_stats *stats, MergeInput &in) {
    std::vector<std::string> &header = in.header, &names = in.names;
    std::string &filt = in.filt;
    std::vector<uint32_t> &filt_off = in.filt_off;
    uint64_t &total_bytes = in.total_bytes;
    names.resize(n_files);
    filt_off.assign(1, 0);
    for (uint32_t f = 0; f < n_files; ++f) {
        std::vector<std::string> h;
        std::string chrom;
        struct stat stt;
        if (!paths[f] || stat(paths[f], &stt) != 0 || !merge_read_head(paths[f], f ? h : header, chrom)) {
            stats->bad_file = f;
            return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot open or read the VCF file %s", paths[f] ? paths[f] : "(null)");
        }
        total_bytes += (uint64_t)stt.st_size;
        size_t tabs = 0, last = 0;
        for (size_t i = 0; i < chrom.size(); ++i) if (chrom[i] == '\t') { ++tabs; last = i; }
        if (tabs != 9) {
            stats->bad_file = f;
            return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "%s: no #CHROM line with one sample column", paths[f]);
        }
        names[f] = chrom.substr(last + 1);
    }
    for (const std::string &h : header) {
        const char key[] = "##FILTER=<ID=";
        if (h.compare(0, sizeof key - 1, key) != 0) continue;
        const size_t a = sizeof key - 1, b = h.find_first_of(",>", a);
        const std::string id = h.substr(a, b == std::string::npos ? std::string::npos : b - a);
        if (id == "PASS") continue;
        filt += id;
        filt_off.push_back((uint32_t)filt.size());
    }
    if (filt_off.size() - 1 > 31) return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "%s: more than 31 filters", paths[0]);
    return SNPGPU_OK;
}

// The lines the kernel left alone ((column, offset) pairs, as the parse kernel reports them): one at a time on the host, by the same
// routine in its wider setting.  Their records (key: the CHROM hash, off and column set) are appended to `extra`.
int merge_host_lines(snpgpu_ctx *ctx, const char *const *paths, const std::vector<uint64_t> &unusual, const MergeInput &in, snpgpu_merge_stats *stats,
                     std::vector<snpgpu_merge_cell> &extra) {
    const uint32_t n_filt = (uint32_t)in.filt_off.size() - 1;
    std::string line;
    for (size_t k = 0; k < unusual.size() / 2; ++k) {
        const uint32_t f = (uint32_t)unusual[2 * k];
        const int fd = open(paths[f], O_RDONLY | O_CLOEXEC);
        uint64_t start = 0;
        const bool got = fd >= 0 && merge_read_line(fd, unusual[2 * k + 1], line, &start);
        if (fd >= 0) close(fd);
        if (!got) { stats->bad_file = f; return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot open or read the VCF file %s", paths[f]); }
        if (line.empty() || line[0] == '#') continue;
        snpgpu_merge_cell c;
        if (line.size() > 0x7FFFFFFFu ||
            !snpgpu_merge_parse_line((const uint8_t *)line.data(), 0, (uint32_t)line.size(), (const uint8_t *)in.filt.data(), in.filt_off.data(), n_filt, false, &c)) {
            stats->bad_file = f;
            stats->bad_offset = start;
            return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "%s: the line at byte %llu is outside the pipeline's own VCF grammar, on which alone the merge is pinned",
                                    paths[f], (unsigned long long)start);
        }
        c.off = start;
        c.column = f;
        extra.push_back(c);
        ++stats->host_lines;
    }
    return SNPGPU_OK;
}

// The contigs in order of first appearance over the columns.  first[i]: column << 40 | offset of the first line that carries contig i.
// rank[i]: its place in that order; contigs: the names in that order, read from those lines.
int merge_contig_order(snpgpu_ctx *ctx, const char *const *paths, const std::vector<uint64_t> &first, snpgpu_merge_stats *stats, std::vector<uint32_t> &rank,
                       std::vector<std::string> &contigs, std::string &all_names, std::vector<uint32_t> &name_off) {
    const uint32_t n = (uint32_t)first.size();
    std::vector<uint32_t> order(n);
    rank.resize(n);
    name_off.assign(1, 0);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return first[a] < first[b]; });
    std::string line;
    for (uint32_t r = 0; r < n; ++r) {
        rank[order[r]] = r;
        const uint32_t f = (uint32_t)(first[order[r]] >> 40);
        const int fd = open(paths[f], O_RDONLY | O_CLOEXEC);
        uint64_t start = 0;
        const bool got = fd >= 0 && merge_read_line(fd, first[order[r]] & ((1ull << 40) - 1), line, &start);
        if (fd >= 0) close(fd);
        if (!got) { stats->bad_file = f; return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot open or read the VCF file %s", paths[f]); }
        contigs.push_back(line.substr(0, line.find('\t')));
        all_names += contigs.back();
        name_off.push_back((uint32_t)all_names.size());
    }
    return SNPGPU_OK;
}

// the header of the merged file
std::string merge_head_text(const MergeInput &in, const std::vector<std::string> &contigs, const char *own_lines, uint32_t own_len) {
    std::string head;
    const std::string pass_line = "##FILTER=<ID=PASS,Description=\"All filters passed\">";
    std::vector<std::string> lines;
    for (const std::string &h : in.header) if (h != pass_line) lines.push_back(h);
    lines.insert(lines.begin() + ((!lines.empty() && lines[0].compare(0, 12, "##fileformat") == 0) ? 1 : 0), pass_line);
    for (const std::string &l : lines) { head += l; head += '\n'; }
    for (const std::string &c : contigs) { head += "##contig=<ID=" + c + ">\n"; }
    if (own_lines && own_len) head.append(own_lines, own_len);
    head += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
    for (const std::string &n : in.names) { head += '\t'; head += n; }
    head += '\n';
    return head;
}

// The text of device buffers to a file: copied back in 16 MiB pieces through the staging ring, each piece written at its place by
// a writer thread.  start(), any number of copy(), finish().
struct MergeWriter {
    struct Piece { uint64_t slot, off, len; };                  // staging buffer, offset in the file, bytes
    static constexpr size_t CHUNK = (size_t)16 << 20;
    snpgpu_ctx *ctx;
    int fd;
    snpgpu_stream_pool *p = nullptr;
    uint64_t R = 0, j = 0;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<Piece> ready;                                   // pieces copied back, waiting for a writer
    std::vector<char> busy;                                     // staging buffer in use (being filled or written)
    bool closing = false, failed = false;
    std::vector<std::thread> writers;
    hipError_t herr = hipSuccess;

    MergeWriter(snpgpu_ctx *c, int f) : ctx(c), fd(f) {}
    ~MergeWriter() { (void)finish(); }
    static uint64_t pieces(uint64_t len) { return (len + CHUNK - 1) / CHUNK; }
    void writer_main() {
        for (;;) {
            Piece pc;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return closing || !ready.empty(); });
                if (ready.empty()) return;
                pc = ready.back();
                ready.pop_back();
            }
            const char *h = (const char *)p->staging[pc.slot];
            bool ok = true;
            for (uint64_t at = 0; at < pc.len && ok;) {
                const ssize_t w = pwrite(fd, h + at, pc.len - at, (off_t)(pc.off + at));
                if (w <= 0) ok = false; else at += (uint64_t)w;
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                busy[pc.slot] = 0;
                if (!ok) failed = true;
            }
            cv.notify_all();
        }
    }
    // n_pieces: how many pieces the copies will come to (at least 1); *n_writers: the threads that run
    int start(uint64_t n_pieces, uint32_t *n_writers) {
        uint32_t n = snpgpu_writer_threads(16);
        if (n > n_pieces) n = (uint32_t)n_pieces;
        if (n < 1) n = 1;
        *n_writers = n;
        const uint32_t n_ring = (uint32_t)(n_pieces < n + 2 ? n_pieces : n + 2);
        const int rc = pool_ensure(ctx, CHUNK, n_ring, 0, 0, 0, 0);
        if (rc) return rc;
        p = ctx->pool;
        R = p->staging.size() < n_ring ? p->staging.size() : n_ring;
        busy.assign(R, 0);
        try {
            for (uint32_t i = 0; i < n; ++i) writers.emplace_back([this] { writer_main(); });
        } catch (const std::exception &) {
            if (writers.empty()) return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "cannot start a writer thread");
        }
        return SNPGPU_OK;
    }
    // d_src[0, len) to the file at file_off (after an error of the device nothing more is copied: see herr)
    void copy(const uint8_t *d_src, uint64_t len, uint64_t file_off) {
        for (uint64_t lo = 0; lo < len && herr == hipSuccess; lo += CHUNK, ++j) {
            const uint64_t slot = j % R;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !busy[slot]; });
                busy[slot] = 1;
            }
            const uint64_t n = len - lo < CHUNK ? len - lo : CHUNK;
            herr = hipMemcpyAsync(p->staging[slot], d_src + lo, n, hipMemcpyDeviceToHost, ctx->stream);
            if (herr == hipSuccess) herr = hipStreamSynchronize(ctx->stream);
            if (herr != hipSuccess) break;
            { std::lock_guard<std::mutex> lk(mu); ready.push_back(Piece{slot, file_off + lo, n}); }
            cv.notify_all();
        }
    }
    // every piece is written (false: a write failed)
    bool finish() {
        { std::lock_guard<std::mutex> lk(mu); closing = true; }
        cv.notify_all();
        for (auto &t : writers) t.join();
        writers.clear();
        return !failed;
    }
};

int merge_vcf_files(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, const char *out_path, const char *own_lines, uint32_t own_len,
                    uint64_t out_cap, snpgpu_merge_stats *stats, const MergeInput *given = nullptr) {
    constexpr uint32_t UNUSUAL_CAP = MERGE_UNUSUAL_CAP;
    HIP_TRY(ctx, snpgpu_enter(ctx));
    hipStream_t st = ctx->stream;
    double t0 = now_s();
    MergeInput own_input;
    if (!given) {
        const int hrc = merge_read_input(ctx, paths, n_files, stats, own_input);
        if (hrc) return hrc;
        given = &own_input;
    }
    const std::string &filt = given->filt;
    const std::vector<uint32_t> &filt_off = given->filt_off;
    const uint64_t total_bytes = given->total_bytes;
    const uint32_t n_filt = (uint32_t)filt_off.size() - 1;

    MergeBuffers mem;
    const uint64_t cell_cap = total_bytes / 56 + UNUSUAL_CAP + 64;      // (no line of the grammar is shorter than 56 bytes)
    if (cell_cap > 0x7FFFFFFEull) return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "too many VCF records for one merge");
    snpgpu_merge_cell *d_cells = nullptr;
    uint64_t *d_ctl = nullptr, *d_unusual = nullptr;
    uint8_t *d_filt = nullptr;
    uint32_t *d_filt_off = nullptr;
    HIP_TRY(ctx, mem.get(&d_cells, cell_cap * sizeof(snpgpu_merge_cell)));
    HIP_TRY(ctx, mem.get(&d_ctl, 64));
    HIP_TRY(ctx, mem.get(&d_unusual, 16ull * UNUSUAL_CAP));
    HIP_TRY(ctx, mem.get(&d_filt, filt.size() + 16));
    HIP_TRY(ctx, mem.get(&d_filt_off, 4 * filt_off.size()));
    HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, 64, st));
    if (!filt.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_filt, filt.data(), filt.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_filt_off, filt_off.data(), 4 * filt_off.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));

    // parse: the files as one stream
    std::vector<int32_t> file_rc(n_files, 0);
    uint64_t ctl[8] = {0};
    int rc = vcf_stream(ctx, paths, n_files, 0, file_rc.data(),
        [&](void *) { return (int)SNPGPU_OK; },
        [&](const uint8_t *d_buf, uint32_t len, uint32_t own_from, const Job &jb) {
            return snpgpu_enqueue_merge_parse(ctx, d_buf, len, own_from, jb.off, jb.file, d_cells, cell_cap, d_ctl, d_unusual, UNUSUAL_CAP, d_filt, d_filt_off, n_filt);
        },
        [&](void *) {
            HIP_TRY(ctx, hipMemcpyAsync(ctl, d_ctl, 64, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            return (int)SNPGPU_OK;
        });
    if (rc) return rc;
    for (uint32_t f = 0; f < n_files; ++f)
        if (file_rc[f]) { stats->bad_file = f; return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot open or read the VCF file %s", paths[f]); }
    if (ctl[2] & 1) return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "more VCF records than the merge made room for");
    if (ctl[1] > UNUSUAL_CAP) return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "%llu lines outside the kernel's grammar: more than the %u the host takes", (unsigned long long)ctl[1], UNUSUAL_CAP);
    uint64_t n_cells = ctl[0];
    // the lines the kernel left alone: one at a time on the host, by the same routine in its wider setting
    if (ctl[1]) {
        std::vector<uint64_t> unusual(2 * ctl[1]);
        HIP_TRY(ctx, hipMemcpy(unusual.data(), d_unusual, 16 * ctl[1], hipMemcpyDeviceToHost));
        std::vector<snpgpu_merge_cell> extra;
        rc = merge_host_lines(ctx, paths, unusual, *given, stats, extra);
        if (rc) return rc;
        if (n_cells + extra.size() > cell_cap) return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "more VCF records than the merge made room for");
        if (!extra.empty()) HIP_TRY(ctx, hipMemcpy(d_cells + n_cells, extra.data(), extra.size() * sizeof(snpgpu_merge_cell), hipMemcpyHostToDevice));
        n_cells += extra.size();
    }
    stats->cells = n_cells;
    stats->seconds_parse = now_s() - t0;
    t0 = now_s();

    // contigs in order of first appearance over the columns, then the site union
    std::vector<std::string> contigs;
    uint32_t n_sites = 0;
    uint64_t *d_keys = nullptr, *d_uniq = nullptr, *d_first = nullptr;
    uint32_t *d_cols = nullptr, *d_off = nullptr, *d_carrier = nullptr, *d_n = nullptr, *d_rank = nullptr, *d_table = nullptr, *d_name_off = nullptr;
    uint8_t *d_names = nullptr;
    if (n_cells) {
        HIP_TRY(ctx, mem.get(&d_keys, 8 * n_cells));
        HIP_TRY(ctx, mem.get(&d_uniq, 8 * n_cells));
        HIP_TRY(ctx, mem.get(&d_cols, 4 * n_cells));
        HIP_TRY(ctx, mem.get(&d_off, 4 * (n_cells + 1)));
        HIP_TRY(ctx, mem.get(&d_carrier, 4 * n_cells));
        HIP_TRY(ctx, mem.get(&d_n, 16));
        rc = snpgpu_enqueue_merge_hash_keys(ctx, d_cells, n_cells, d_keys, d_cols);
        if (rc) return rc;
        rc = snpgpu_merge_sites_dev(ctx, d_keys, d_cols, (uint32_t)n_cells, d_uniq, d_off, d_carrier, d_n);
        if (rc) return rc;
        uint32_t n_u[2] = {0, 0};
        HIP_TRY(ctx, hipMemcpyAsync(n_u, d_n, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        HIP_TRY(ctx, mem.get(&d_first, 8ull * n_u[0]));
        HIP_TRY(ctx, mem.get(&d_rank, 4ull * n_u[0]));
        HIP_TRY(ctx, hipMemsetAsync(d_first, 0xFF, 8ull * n_u[0], st));
        rc = snpgpu_enqueue_merge_contig_first(ctx, d_cells, n_cells, d_uniq, d_n, d_first);
        if (rc) return rc;
        std::vector<uint64_t> first(n_u[0]);
        HIP_TRY(ctx, hipMemcpyAsync(first.data(), d_first, 8ull * n_u[0], hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        std::vector<uint32_t> rank, name_off;
        std::string all_names;
        rc = merge_contig_order(ctx, paths, first, stats, rank, contigs, all_names, name_off);
        if (rc) return rc;
        HIP_TRY(ctx, mem.get(&d_names, all_names.size() + 16));
        HIP_TRY(ctx, mem.get(&d_name_off, 4 * name_off.size()));
        HIP_TRY(ctx, hipMemcpyAsync(d_names, all_names.data(), all_names.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_name_off, name_off.data(), 4 * name_off.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_rank, rank.data(), 4ull * n_u[0], hipMemcpyHostToDevice, st));
        rc = snpgpu_enqueue_merge_site_keys(ctx, d_cells, n_cells, d_rank, d_keys, d_cols);
        if (rc) return rc;
        rc = snpgpu_merge_sites_dev(ctx, d_keys, d_cols, (uint32_t)n_cells, d_uniq, d_off, d_carrier, d_n);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(n_u, d_n, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));              // (the host vectors above were copied from)
        n_sites = n_u[0];
        if ((uint64_t)n_sites * n_files > 0xFFFFFFFFFFull) return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "too many sample cells for one merge");
        HIP_TRY(ctx, mem.get(&d_table, 4ull * n_sites * n_files));
        HIP_TRY(ctx, hipMemsetAsync(d_table, 0, 4ull * n_sites * n_files, st));
        rc = snpgpu_enqueue_merge_scatter(ctx, d_cells, n_cells, d_uniq, d_n, n_files, d_table, d_ctl);
        if (rc) return rc;
    }
    stats->sites = n_sites;

    const std::string head = merge_head_text(*given, contigs, own_lines, own_len);

    // rows: the lengths and offsets of all sites (16 bytes a site) ...
    uint64_t out_bytes = 0;
    uint64_t *d_row_len = nullptr, *d_row_end = nullptr, *d_scan = nullptr;
    std::vector<uint64_t> row_end;
    if (n_sites) {
        HIP_TRY(ctx, mem.get(&d_row_len, 8ull * n_sites));
        HIP_TRY(ctx, mem.get(&d_row_end, 8ull * n_sites));
        HIP_TRY(ctx, mem.get(&d_scan, 8 * (snpgpu_merge_rows_scan_words(n_sites) + 1)));
        rc = snpgpu_enqueue_merge_rows(ctx, 0, d_cells, d_table, n_files, d_uniq, n_sites, 0, n_sites, 0, d_names, d_name_off, d_filt, d_filt_off, d_row_len, d_row_end, d_scan,
                                       nullptr, d_ctl);
        if (rc) return rc;
        row_end.resize(n_sites);
        HIP_TRY(ctx, hipMemcpyAsync(row_end.data(), d_row_end, 8ull * n_sites, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctl, d_ctl, 64, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        out_bytes = row_end[n_sites - 1];
        if (ctl[2] & 2) {
            snpgpu_merge_cell c;
            HIP_TRY(ctx, hipMemcpy(&c, d_cells + ctl[3], sizeof c, hipMemcpyDeviceToHost));
            stats->bad_file = c.column;
            stats->bad_offset = c.off;
            return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "%s: the position of the line at byte %llu comes twice in the file", paths[c.column], (unsigned long long)c.off);
        }
        if (ctl[2] & 4) return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "records of different REF at one position: outside the grammar the merge is pinned on");
    }
    // ... and the rounds: as many whole rows as the output buffer holds (a row longer than the buffer is a round of its own,
    // and the buffer is as long as the longest round)
    struct Round { uint32_t lo, hi; uint64_t base, len; };
    std::vector<Round> rounds;
    uint64_t buf_bytes = 0;
    for (uint32_t lo = 0; lo < n_sites;) {
        const uint64_t base = lo ? row_end[lo - 1] : 0;
        uint32_t hi = (uint32_t)(std::upper_bound(row_end.begin() + lo, row_end.end(), base + out_cap) - row_end.begin());
        if (hi == lo) hi = lo + 1;
        rounds.push_back(Round{lo, hi, base, row_end[hi - 1] - base});
        if (rounds.back().len > buf_bytes) buf_bytes = rounds.back().len;
        lo = hi;
    }
    std::vector<uint64_t>().swap(row_end);
    stats->rounds = (uint32_t)(rounds.size() < 0xFFFFFFFFu ? rounds.size() : 0xFFFFFFFFu);
    uint8_t *d_out = nullptr;
    if (n_sites) HIP_TRY(ctx, mem.get(&d_out, buf_bytes + 16));
    stats->seconds_merge = now_s() - t0;
    t0 = now_s();

    // the file: each round's text comes back in pieces through the staging ring, writer threads pwrite each piece at its place
    // (the time of the rounds' text kernels is in seconds_write: they run between the copies)
    const int fd = open(out_path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd < 0) return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot create %s", out_path);
    bool io_ok = true;
    for (size_t at = 0; at < head.size() && io_ok;) {
        const ssize_t w = pwrite(fd, head.data() + at, head.size() - at, (off_t)at);
        if (w <= 0) io_ok = false; else at += (size_t)w;
    }
    uint64_t n_pieces = 0;
    for (const Round &r : rounds) n_pieces += MergeWriter::pieces(r.len);
    rc = SNPGPU_OK;
    stats->writer_threads = 1;
    if (n_pieces) {
        MergeWriter wr(ctx, fd);
        rc = wr.start(n_pieces, &stats->writer_threads);
        if (rc) { close(fd); return rc; }
        int krc = SNPGPU_OK;
        for (size_t r = 0; r < rounds.size() && wr.herr == hipSuccess && krc == SNPGPU_OK; ++r) {
            const Round &rd = rounds[r];                        // (the copies of the round before are complete: the buffer is free)
            krc = snpgpu_enqueue_merge_rows(ctx, 1, d_cells, d_table, n_files, d_uniq, n_sites, rd.lo, rd.hi, rd.base, d_names, d_name_off, d_filt, d_filt_off, d_row_len,
                                            d_row_end, d_scan, d_out, d_ctl);
            if (krc == SNPGPU_OK) wr.copy(d_out, rd.len, head.size() + rd.base);
        }
        if (!wr.finish()) io_ok = false;
        if (krc) rc = krc;
        else if (wr.herr != hipSuccess) rc = snpgpu_set_error(ctx, SNPGPU_E_HIP, "copying the merged text back failed: %s", hipGetErrorString(wr.herr));
    }
    if (close(fd) != 0) io_ok = false;
    if (rc) return rc;
    if (!io_ok) return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot write %s", out_path);
    stats->bytes = head.size() + out_bytes;
    stats->seconds_write = now_s() - t0;
    return SNPGPU_OK;
}

// ---- merge_vcfs in bounded memory -----------------------------------------------------------------------------------------------
// The plan (include/snpgpu.h: snpgpu_merge_plan).  Everything is a figure of (n_files, n_sites, input bytes, budget, output buffer).
constexpr uint64_t MERGE_MAX_RECORDS = 0x7FFFFFFEull;
constexpr uint64_t MERGE_STREAM_BYTES = 3 * (((uint64_t)16 << 20) + 256) + 512;     // vcf_stream's piece buffers
constexpr uint64_t MERGE_SMALL_BYTES = (16ull * MERGE_UNUSUAL_CAP) + (64 << 10);     // the list of the host's lines; control words, filters, contigs
constexpr uint64_t MERGE_MIN_KEYS = 4096, MERGE_MAX_KEYS = 1ull << 30;
constexpr uint32_t MERGE_EXTRA_BUF = 1024;                   // records of host-parsed lines go to their slots this many at a time
constexpr uint64_t MERGE_NO_BUDGET = 1ull << 62;

struct MergePlan {
    snpgpu_merge_passes p;
    uint64_t key_cap;               // keys a batch of the key pass holds
    uint64_t out_buf;               // bytes of the output buffer of a site round
};

inline uint64_t merge_row_estimate(uint32_t n_files) { return 256 + 48ull * n_files; }
inline uint64_t merge_min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
// the arrays of one sort + unique over m keys: keys, zeros, unique keys, offsets, carriers, the counts, the sort's workspace
inline uint64_t merge_fold_bytes(uint64_t m) { return 28 * m + 4 + 16 + 6 * 256 + snpgpu_merge_sites_ws_bytes(m); }

// the single pass by the dense bound; UINT64_MAX where it cannot run at any budget
uint64_t merge_single_bytes(uint32_t n_files, uint64_t total_bytes, uint64_t out_cap) {
    const uint64_t cap = total_bytes / 56 + MERGE_UNUSUAL_CAP + 64;
    if (cap > MERGE_MAX_RECORDS) return UINT64_MAX;
    const uint64_t sites = (cap + n_files - 1) / n_files;
    return MERGE_STREAM_BYTES + MERGE_SMALL_BYTES + cap * sizeof(snpgpu_merge_cell) + merge_fold_bytes(cap) + 4 * cap /* the table */ + 16 * sites +
           8 * (snpgpu_merge_rows_scan_words((uint32_t)sites) + 1) + merge_min64(out_cap, sites * merge_row_estimate(n_files)) + 16;
}

uint64_t merge_round_out_bytes(uint32_t n_files, uint64_t s, uint64_t out_cap) {
    const uint64_t row = merge_row_estimate(n_files);
    return s * row < out_cap ? s * row : (out_cap > row ? out_cap : row);
}

// the bounded form with rounds of s sites: the key pass (a batch and its fold into the union, the union before and after) and a
// site round (the union, the slots, the row arrays, the output buffer), beside what both hold.  The key pass's arrays are freed
// before the first round: the plan counts both all the same, so that every number of sites a round has a budget of its own
uint64_t merge_bounded_bytes(uint32_t n_files, uint64_t n_sites, uint64_t key_cap, uint64_t s, uint64_t out_cap) {
    const uint64_t key_pass = key_cap * (sizeof(snpgpu_merge_key) + 4) + merge_fold_bytes(key_cap + n_sites) + 16 * n_sites;
    const uint64_t round = 8 * n_sites + s * n_files * (sizeof(snpgpu_merge_cell) + 4) + 16 * s + 8 * (snpgpu_merge_rows_scan_words((uint32_t)s) + 1) +
                           merge_round_out_bytes(n_files, s, out_cap) + 16 + MERGE_EXTRA_BUF * sizeof(snpgpu_merge_cell);
    return MERGE_STREAM_BYTES + MERGE_SMALL_BYTES + key_pass + round;
}

// SNPGPU_OK, or SNPGPU_E_NOMEM with pl->p.device_bytes = the bytes a round of one site needs
int merge_plan(uint32_t n_files, uint64_t n_sites, uint64_t total_bytes, uint64_t budget, uint64_t out_cap, MergePlan *pl) {
    *pl = MergePlan{};
    if (!budget) budget = MERGE_NO_BUDGET;
    if (budget > MERGE_NO_BUDGET) budget = MERGE_NO_BUDGET;
    const uint64_t always = MERGE_STREAM_BYTES + MERGE_SMALL_BYTES;
    uint64_t key_cap = (budget > always ? budget - always : 0) / 8 / 128;      // (about 128 bytes a key: its 24, and its share of the fold)
    key_cap = key_cap < MERGE_MIN_KEYS ? MERGE_MIN_KEYS : key_cap > MERGE_MAX_KEYS ? MERGE_MAX_KEYS : key_cap;
    pl->key_cap = key_cap;
    const uint64_t sites = n_sites > 0xFFFFFFFEull ? 0xFFFFFFFEull : n_sites;
    const uint64_t single = merge_single_bytes(n_files, total_bytes, out_cap);
    const bool single_fits = single <= budget;
    // the most sites a round holds
    uint64_t lo = 0, hi = MERGE_MAX_RECORDS / n_files;         // (need(lo) fits, or lo is 0)
    if (hi > 0xFFFFFFFEull) hi = 0xFFFFFFFEull;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (merge_bounded_bytes(n_files, sites, key_cap, mid, out_cap) <= budget) lo = mid; else hi = mid - 1;
    }
    if (single_fits) {
        pl->p.input_passes = 1;
        pl->p.site_rounds = 0;
        pl->p.sites_per_round = lo > sites ? lo : sites;       // (the one round holds every site)
        pl->p.device_bytes = single;
        return SNPGPU_OK;
    }
    if (lo == 0) {
        pl->p.device_bytes = merge_bounded_bytes(n_files, sites, MERGE_MIN_KEYS, 1, out_cap);
        return SNPGPU_E_NOMEM;
    }
    if (single != UINT64_MAX && sites >= 2 && lo >= sites) lo = sites - 1;     // (the round of all sites is the single pass, and that does not fit)
    pl->p.sites_per_round = lo;
    pl->p.site_rounds = (uint32_t)((sites + lo - 1) / lo);
    pl->p.input_passes = 1 + pl->p.site_rounds;
    pl->p.device_bytes = merge_bounded_bytes(n_files, sites, key_cap, lo, out_cap);
    pl->out_buf = merge_round_out_bytes(n_files, lo, out_cap);
    return SNPGPU_OK;
}

// the merged file under a sibling name until it is whole: renamed at the end, removed on every other way out
struct MergeTemp {
    std::string path;
    int fd = -1;
    ~MergeTemp() {
        if (fd >= 0) close(fd);
        if (!path.empty()) (void)unlink(path.c_str());
    }
    bool create(const char *out_path) {
        static std::atomic<uint32_t> serial{0};
        for (int k = 0; k < 100 && fd < 0; ++k) {
            char tail[64];
            snprintf(tail, sizeof tail, ".snpgpu-merge.%ld.%u", (long)getpid(), serial.fetch_add(1));
            path = std::string(out_path) + tail;
            fd = open(path.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0666);
            if (fd < 0 && errno != EEXIST) break;
        }
        if (fd < 0) path.clear();
        return fd >= 0;
    }
    bool commit(const char *out_path) {
        const bool closed = close(fd) == 0;
        fd = -1;
        if (!closed || rename(path.c_str(), out_path) != 0) return false;
        path.clear();
        return true;
    }
};

int merge_vcf_files_bounded(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, const char *out_path, const char *own_lines, uint32_t own_len,
                            uint64_t out_cap, uint64_t budget, const MergeInput &in, snpgpu_merge_stats *stats, snpgpu_merge_passes *passes) {
    hipStream_t st = ctx->stream;
    double t0 = now_s();
    const uint32_t n_filt = (uint32_t)in.filt_off.size() - 1;
    MergePlan pl;
    auto no_memory = [&](const MergePlan &q) {
        *passes = q.p;
        return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "merge_vcfs needs %llu bytes of device memory for its key pass and a round of one site of %u columns: the budget is %llu",
                                (unsigned long long)q.p.device_bytes, n_files, (unsigned long long)budget);
    };
    if (merge_plan(n_files, 1, in.total_bytes, budget, out_cap, &pl)) return no_memory(pl);      // (before anything is read: no number of sites makes it fit)
    const uint64_t key_cap = pl.key_cap;

    MergeBuffers mem;
    snpgpu_merge_key *d_krec = nullptr;
    uint64_t *d_ctl = nullptr, *d_unusual = nullptr;
    uint8_t *d_filt = nullptr;
    uint32_t *d_filt_off = nullptr;
    HIP_TRY(ctx, mem.get(&d_krec, key_cap * sizeof(snpgpu_merge_key)));
    HIP_TRY(ctx, mem.get(&d_ctl, 64));
    HIP_TRY(ctx, mem.get(&d_unusual, 16ull * MERGE_UNUSUAL_CAP));
    HIP_TRY(ctx, mem.get(&d_filt, in.filt.size() + 16));
    HIP_TRY(ctx, mem.get(&d_filt_off, 4 * in.filt_off.size()));
    HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, 64, st));
    if (!in.filt.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_filt, in.filt.data(), in.filt.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_filt_off, in.filt_off.data(), 4 * in.filt_off.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));

    // ---- the key pass: batches of keys, each sorted, uniqued and folded into the running union ----
    std::unordered_map<uint64_t, uint32_t> id_of;               // CHROM hash -> the contig's number for now (order of appearance over the batches)
    std::vector<uint64_t> hash_of, first_of;                    // per such number: its hash, the first (column << 40 | offset) that carries it
    uint64_t *d_union = nullptr;                                // (number << 32) | POS, ascending
    uint32_t n_union = 0;
    std::vector<uint64_t> unusual;                              // (column, offset) of the lines left to the host, over all batches
    uint64_t n_unusual = 0;
    auto fold = [&](uint32_t n) -> int {                        // d_krec[0, n) into the union
        if (!n) return (int)SNPGPU_OK;
        const uint64_t m = (uint64_t)n + n_union;
        if (m > 0x7FFFFFFFull) return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "too many sites for one merge");
        MergeBuffers tmp;
        uint64_t *d_keys = nullptr, *d_uniq = nullptr, *d_first = nullptr, *d_new = nullptr;
        uint32_t *d_zeros = nullptr, *d_off = nullptr, *d_carrier = nullptr, *d_n = nullptr, *d_which = nullptr, *d_id = nullptr;
        void *d_ws = nullptr;
        HIP_TRY(ctx, tmp.get(&d_keys, 8 * m));
        HIP_TRY(ctx, tmp.get(&d_uniq, 8 * m));
        HIP_TRY(ctx, tmp.get(&d_zeros, 4 * m));
        HIP_TRY(ctx, tmp.get(&d_off, 4 * (m + 1)));
        HIP_TRY(ctx, tmp.get(&d_carrier, 4 * m));
        HIP_TRY(ctx, tmp.get(&d_n, 16));
        HIP_TRY(ctx, tmp.get(&d_which, 4ull * n));
        HIP_TRY(ctx, tmp.get(&d_ws, snpgpu_merge_sites_ws_bytes(m)));
        int rc = snpgpu_enqueue_merge_key_hashes(ctx, d_krec, n, d_keys, d_zeros);
        if (rc) return rc;
        rc = snpgpu_enqueue_merge_sites_ws(ctx, d_keys, d_zeros, n, d_uniq, d_off, d_carrier, d_n, d_ws);
        if (rc) return rc;
        uint32_t n_u[2] = {0, 0};
        HIP_TRY(ctx, hipMemcpyAsync(n_u, d_n, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        HIP_TRY(ctx, tmp.get(&d_first, 8ull * n_u[0]));
        HIP_TRY(ctx, tmp.get(&d_id, 4ull * n_u[0]));
        HIP_TRY(ctx, hipMemsetAsync(d_first, 0xFF, 8ull * n_u[0], st));
        rc = snpgpu_enqueue_merge_key_first(ctx, d_krec, n, d_uniq, d_n, d_which, d_first);
        if (rc) return rc;
        std::vector<uint64_t> uniq(n_u[0]), first(n_u[0]);
        std::vector<uint32_t> id(n_u[0]);
        HIP_TRY(ctx, hipMemcpyAsync(uniq.data(), d_uniq, 8ull * n_u[0], hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(first.data(), d_first, 8ull * n_u[0], hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (uint32_t k = 0; k < n_u[0]; ++k) {
            const auto at = id_of.emplace(uniq[k], (uint32_t)hash_of.size());
            if (at.second) { hash_of.push_back(uniq[k]); first_of.push_back(UINT64_MAX); }
            id[k] = at.first->second;
            if (first[k] < first_of[id[k]]) first_of[id[k]] = first[k];
        }
        HIP_TRY(ctx, hipMemcpyAsync(d_id, id.data(), 4ull * n_u[0], hipMemcpyHostToDevice, st));
        rc = snpgpu_enqueue_merge_key_sites(ctx, d_krec, n, d_which, d_id, d_keys, d_zeros);
        if (rc) return rc;
        if (n_union) {
            HIP_TRY(ctx, hipMemcpyAsync(d_keys + n, d_union, 8ull * n_union, hipMemcpyDeviceToDevice, st));
            HIP_TRY(ctx, hipMemsetAsync(d_zeros + n, 0, 4ull * n_union, st));
        }
        rc = snpgpu_enqueue_merge_sites_ws(ctx, d_keys, d_zeros, (uint32_t)m, d_uniq, d_off, d_carrier, d_n, d_ws);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(n_u, d_n, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));                 // (id was copied from)
        HIP_TRY(ctx, mem.get(&d_new, 8ull * n_u[0]));
        HIP_TRY(ctx, hipMemcpyAsync(d_new, d_uniq, 8ull * n_u[0], hipMemcpyDeviceToDevice, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        mem.release(d_union);
        d_union = d_new;
        n_union = n_u[0];
        return (int)SNPGPU_OK;
    };
    uint64_t pending = 0;                                       // the most keys the launches since the last flush may have left
    auto flush = [&]() -> int {                                 // the batch so far: its keys into the union, its other lines to the list
        uint64_t ctl[8];
        HIP_TRY(ctx, hipMemcpyAsync(ctl, d_ctl, 64, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        pending = 0;
        if (ctl[2] & 1) return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "more VCF records than the merge made room for");
        n_unusual += ctl[1];
        if (n_unusual > MERGE_UNUSUAL_CAP)
            return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "%llu lines outside the kernel's grammar: more than the %u the host takes", (unsigned long long)n_unusual, MERGE_UNUSUAL_CAP);
        if (ctl[1]) {
            const size_t at = unusual.size();
            unusual.resize(at + 2 * ctl[1]);
            HIP_TRY(ctx, hipMemcpy(unusual.data() + at, d_unusual, 16 * ctl[1], hipMemcpyDeviceToHost));
        }
        const int rc = fold((uint32_t)ctl[0]);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, 16, st));
        return (int)SNPGPU_OK;
    };
    std::vector<int32_t> file_rc(n_files, 0);
    int rc = vcf_stream(ctx, paths, n_files, 0, file_rc.data(),
        [&](void *) { return (int)SNPGPU_OK; },
        [&](const uint8_t *d_buf, uint32_t len, uint32_t own_from, const Job &jb) {
            // the piece in parts of whole tiles, each no longer than the batch has room for (a line of the grammar has 56 bytes or more)
            for (uint32_t a = own_from; a < len;) {
                const uint64_t room = key_cap - pending;
                const uint64_t take = room > 2 ? (room - 2) * 56 / SNPGPU_VCF_TILE * SNPGPU_VCF_TILE : 0;
                if (!take) {
                    const int frc = flush();
                    if (frc) return frc;
                    continue;
                }
                const uint32_t b = len - a <= take ? len : a + (uint32_t)take;
                const int krc = a == own_from
                    ? snpgpu_enqueue_merge_lines(ctx, d_buf, b, own_from, jb.off, jb.file, d_krec, key_cap, nullptr, d_ctl, d_unusual, MERGE_UNUSUAL_CAP, d_filt, d_filt_off, n_filt)
                    : snpgpu_enqueue_merge_lines(ctx, d_buf + a - SNPGPU_VCF_LOOK, b - a + SNPGPU_VCF_LOOK, SNPGPU_VCF_LOOK, jb.off + a - SNPGPU_VCF_LOOK, jb.file, d_krec,
                                                 key_cap, nullptr, d_ctl, d_unusual, MERGE_UNUSUAL_CAP, d_filt, d_filt_off, n_filt);
                if (krc) return krc;
                pending += (b - a) / 56 + 2;
                a = b;
            }
            return (int)SNPGPU_OK;
        },
        [&](void *) { return flush(); });
    if (rc) return rc;
    for (uint32_t f = 0; f < n_files; ++f)
        if (file_rc[f]) { stats->bad_file = f; return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot open or read the VCF file %s", paths[f]); }
    // the lines the kernel left alone: parsed once, here; their records stay on the host and go to their slots in their round
    std::vector<snpgpu_merge_cell> extra;
    rc = merge_host_lines(ctx, paths, unusual, in, stats, extra);
    if (rc) return rc;
    for (size_t at = 0; at < extra.size();) {
        const size_t n = extra.size() - at < key_cap ? extra.size() - at : (size_t)key_cap;
        std::vector<snpgpu_merge_key> rec(n);
        for (size_t k = 0; k < n; ++k) rec[k] = snpgpu_merge_key{extra[at + k].key, extra[at + k].off, extra[at + k].pos, extra[at + k].column};
        HIP_TRY(ctx, hipMemcpy(d_krec, rec.data(), n * sizeof(snpgpu_merge_key), hipMemcpyHostToDevice));
        rc = fold((uint32_t)n);
        if (rc) return rc;
        at += n;
    }
    mem.release(d_krec);
    mem.release(d_unusual);
    d_krec = nullptr;
    d_unusual = nullptr;

    // the contigs in order of first appearance over the columns; the union under those numbers, sorted once more
    const uint32_t n_sites = n_union, n_contigs = (uint32_t)hash_of.size();
    std::vector<uint32_t> rank, name_off;
    std::vector<std::string> contigs;
    std::string all_names;
    rc = merge_contig_order(ctx, paths, first_of, stats, rank, contigs, all_names, name_off);
    if (rc) return rc;
    std::vector<uint64_t> sites(n_sites);
    uint64_t *d_sites = nullptr, *d_hashes = nullptr;
    uint32_t *d_rank = nullptr, *d_name_off = nullptr;
    uint8_t *d_names = nullptr;
    if (n_sites) {
        std::vector<uint32_t> by_hash(n_contigs), rank_by_hash(n_contigs);
        std::vector<uint64_t> hashes(n_contigs);
        for (uint32_t i = 0; i < n_contigs; ++i) by_hash[i] = i;
        std::sort(by_hash.begin(), by_hash.end(), [&](uint32_t a, uint32_t b) { return hash_of[a] < hash_of[b]; });
        for (uint32_t i = 0; i < n_contigs; ++i) { hashes[i] = hash_of[by_hash[i]]; rank_by_hash[i] = rank[by_hash[i]]; }
        MergeBuffers tmp;
        uint64_t *d_uniq = nullptr;
        uint32_t *d_zeros = nullptr, *d_off = nullptr, *d_carrier = nullptr, *d_n = nullptr, *d_rank_of = nullptr;
        void *d_ws = nullptr;
        HIP_TRY(ctx, tmp.get(&d_uniq, 8ull * n_sites));
        HIP_TRY(ctx, tmp.get(&d_zeros, 4ull * n_sites));
        HIP_TRY(ctx, tmp.get(&d_off, 4ull * (n_sites + 1)));
        HIP_TRY(ctx, tmp.get(&d_carrier, 4ull * n_sites));
        HIP_TRY(ctx, tmp.get(&d_n, 16));
        HIP_TRY(ctx, tmp.get(&d_rank_of, 4ull * n_contigs));
        HIP_TRY(ctx, tmp.get(&d_ws, snpgpu_merge_sites_ws_bytes(n_sites)));
        HIP_TRY(ctx, mem.get(&d_hashes, 8ull * n_contigs));
        HIP_TRY(ctx, mem.get(&d_rank, 4ull * n_contigs));
        HIP_TRY(ctx, mem.get(&d_names, all_names.size() + 16));
        HIP_TRY(ctx, mem.get(&d_name_off, 4 * name_off.size()));
        HIP_TRY(ctx, hipMemcpyAsync(d_rank_of, rank.data(), 4ull * n_contigs, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_hashes, hashes.data(), 8ull * n_contigs, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_rank, rank_by_hash.data(), 4ull * n_contigs, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_names, all_names.data(), all_names.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_name_off, name_off.data(), 4 * name_off.size(), hipMemcpyHostToDevice, st));
        rc = snpgpu_enqueue_merge_key_rank(ctx, d_union, n_sites, d_rank_of, d_zeros);
        if (rc) return rc;
        rc = snpgpu_enqueue_merge_sites_ws(ctx, d_union, d_zeros, n_sites, d_uniq, d_off, d_carrier, d_n, d_ws);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(d_union, d_uniq, 8ull * n_sites, hipMemcpyDeviceToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(sites.data(), d_uniq, 8ull * n_sites, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));                 // (the host vectors above were copied from)
        d_sites = d_union;
    }
    stats->sites = n_sites;
    for (snpgpu_merge_cell &c : extra) {                        // the host's records: their site's key and rank
        c.key = ((uint64_t)rank[id_of[c.key]] << 32) | c.pos;
        c.idx = (uint32_t)(std::lower_bound(sites.begin(), sites.end(), c.key) - sites.begin());
    }
    std::sort(extra.begin(), extra.end(), [](const snpgpu_merge_cell &a, const snpgpu_merge_cell &b) { return a.idx < b.idx; });

    if (merge_plan(n_files, n_sites, in.total_bytes, budget, out_cap, &pl)) return no_memory(pl);
    *passes = pl.p;
    const uint32_t per_round = (uint32_t)pl.p.sites_per_round;
    stats->seconds_parse = now_s() - t0;
    t0 = now_s();

    // ---- the site rounds ----
    const std::string head = merge_head_text(in, contigs, own_lines, own_len);
    MergeTemp tmp_file;
    if (!tmp_file.create(out_path)) return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot create %s", out_path);
    bool io_ok = true;
    for (size_t at = 0; at < head.size() && io_ok;) {
        const ssize_t w = pwrite(tmp_file.fd, head.data() + at, head.size() - at, (off_t)at);
        if (w <= 0) io_ok = false; else at += (size_t)w;
    }
    snpgpu_merge_cell *d_cells = nullptr, *d_extra = nullptr;
    uint32_t *d_table = nullptr;
    uint64_t *d_row_len = nullptr, *d_row_end = nullptr, *d_scan = nullptr;
    uint8_t *d_out = nullptr;
    uint64_t out_bytes = pl.out_buf, text_bytes = 0, n_rounds = 0;
    if (n_sites) {
        const uint64_t slots = (uint64_t)per_round * n_files;
        HIP_TRY(ctx, mem.get(&d_cells, slots * sizeof(snpgpu_merge_cell)));
        HIP_TRY(ctx, mem.get(&d_table, 4 * slots));
        HIP_TRY(ctx, mem.get(&d_row_len, 8ull * per_round));
        HIP_TRY(ctx, mem.get(&d_row_end, 8ull * per_round));
        HIP_TRY(ctx, mem.get(&d_scan, 8 * (snpgpu_merge_rows_scan_words(per_round) + 1)));
        HIP_TRY(ctx, mem.get(&d_out, out_bytes + 16));
        if (!extra.empty()) HIP_TRY(ctx, mem.get(&d_extra, MERGE_EXTRA_BUF * sizeof(snpgpu_merge_cell)));
    }
    stats->seconds_merge = now_s() - t0;
    size_t next_extra = 0;
    std::vector<uint64_t> row_end;
    stats->writer_threads = 1;
    for (uint32_t lo = 0; lo < n_sites && io_ok; lo += per_round) {
        t0 = now_s();
        const uint32_t hi = n_sites - lo < per_round ? n_sites : lo + per_round, n_local = hi - lo;
        HIP_TRY(ctx, hipMemsetAsync(d_table, 0, 4ull * n_local * n_files, st));
        HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, 64, st));
        const snpgpu_merge_range range{d_hashes, d_rank, d_sites, n_contigs, n_sites, lo, hi, n_files, d_cells, d_table};
        rc = vcf_stream(ctx, paths, n_files, 0, file_rc.data(),
            [&](void *) { return (int)SNPGPU_OK; },
            [&](const uint8_t *d_buf, uint32_t len, uint32_t own_from, const Job &jb) {
                return snpgpu_enqueue_merge_lines(ctx, d_buf, len, own_from, jb.off, jb.file, nullptr, 0, &range, d_ctl, nullptr, 0, d_filt, d_filt_off, n_filt);
            },
            [&](void *) {
                HIP_TRY(ctx, hipStreamSynchronize(st));
                return (int)SNPGPU_OK;
            });
        if (rc) return rc;
        for (uint32_t f = 0; f < n_files; ++f)
            if (file_rc[f]) { stats->bad_file = f; return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot open or read the VCF file %s", paths[f]); }
        while (next_extra < extra.size() && extra[next_extra].idx < hi) {
            size_t n = 0;
            while (n < MERGE_EXTRA_BUF && next_extra + n < extra.size() && extra[next_extra + n].idx < hi) ++n;
            HIP_TRY(ctx, hipMemcpy(d_extra, extra.data() + next_extra, n * sizeof(snpgpu_merge_cell), hipMemcpyHostToDevice));
            rc = snpgpu_enqueue_merge_place(ctx, d_extra, (uint32_t)n, lo, n_files, d_cells, d_table, d_ctl);
            if (rc) return rc;
            HIP_TRY(ctx, hipStreamSynchronize(st));
            next_extra += n;
        }
        stats->seconds_parse += now_s() - t0;
        t0 = now_s();
        // rows: the lengths and offsets of the round's sites, and the errors only the records show
        rc = snpgpu_enqueue_merge_rows(ctx, 0, d_cells, d_table, n_files, d_sites + lo, n_local, 0, n_local, 0, d_names, d_name_off, d_filt, d_filt_off, d_row_len, d_row_end,
                                       d_scan, nullptr, d_ctl);
        if (rc) return rc;
        uint64_t ctl[8];
        row_end.resize(n_local);
        HIP_TRY(ctx, hipMemcpyAsync(row_end.data(), d_row_end, 8ull * n_local, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctl, d_ctl, 64, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (ctl[2] & 2) {
            const uint32_t f = (uint32_t)(ctl[3] >> 40);
            const uint64_t off = ctl[3] & ((1ull << 40) - 1);
            stats->bad_file = f;
            stats->bad_offset = off;
            return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "%s: the position of the line at byte %llu comes twice in the file", paths[f], (unsigned long long)off);
        }
        if (ctl[2] & 4) return snpgpu_set_error(ctx, SNPGPU_E_UNSUPPORTED, "records of different REF at one position: outside the grammar the merge is pinned on");
        stats->cells += ctl[0];
        // the text in ranges of whole rows that the output buffer holds (a row longer than the buffer: the buffer grows to it)
        struct Round { uint32_t lo, hi; uint64_t base, len; };
        std::vector<Round> rounds;
        uint64_t longest = 0, n_pieces = 0;
        for (uint32_t a = 0; a < n_local;) {
            const uint64_t base = a ? row_end[a - 1] : 0;
            uint32_t b = (uint32_t)(std::upper_bound(row_end.begin() + a, row_end.end(), base + pl.out_buf) - row_end.begin());
            if (b == a) b = a + 1;
            rounds.push_back(Round{a, b, base, row_end[b - 1] - base});
            if (rounds.back().len > longest) longest = rounds.back().len;
            n_pieces += MergeWriter::pieces(rounds.back().len);
            a = b;
        }
        if (longest > out_bytes) {
            mem.release(d_out);
            d_out = nullptr;
            HIP_TRY(ctx, mem.get(&d_out, longest + 16));
            out_bytes = longest;
        }
        n_rounds += rounds.size();
        stats->seconds_merge += now_s() - t0;
        t0 = now_s();
        {
            MergeWriter wr(ctx, tmp_file.fd);
            uint32_t n_writers = 1;
            rc = wr.start(n_pieces, &n_writers);
            if (rc) return rc;
            if (n_writers > stats->writer_threads) stats->writer_threads = n_writers;
            int krc = SNPGPU_OK;
            for (size_t r = 0; r < rounds.size() && wr.herr == hipSuccess && krc == SNPGPU_OK; ++r) {
                const Round &rd = rounds[r];
                krc = snpgpu_enqueue_merge_rows(ctx, 1, d_cells, d_table, n_files, d_sites + lo, n_local, rd.lo, rd.hi, rd.base, d_names, d_name_off, d_filt, d_filt_off,
                                                d_row_len, d_row_end, d_scan, d_out, d_ctl);
                if (krc == SNPGPU_OK) wr.copy(d_out, rd.len, head.size() + text_bytes + rd.base);
            }
            if (!wr.finish()) io_ok = false;
            if (krc) return krc;
            if (wr.herr != hipSuccess) return snpgpu_set_error(ctx, SNPGPU_E_HIP, "copying the merged text back failed: %s", hipGetErrorString(wr.herr));
        }
        text_bytes += row_end[n_local - 1];
        stats->seconds_write += now_s() - t0;
    }
    stats->rounds = (uint32_t)(n_rounds < 0xFFFFFFFFu ? n_rounds : 0xFFFFFFFFu);
    if (!io_ok || !tmp_file.commit(out_path)) return snpgpu_set_error(ctx, SNPGPU_E_IO, "cannot write %s", out_path);
    stats->bytes = head.size() + text_bytes;
    return SNPGPU_OK;
}

// the route by the plan: the single pass where it fits the budget, else the bounded form
int merge_vcf_files_planned(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, const char *out_path, const char *own_lines, uint32_t own_len,
                            const snpgpu_merge_opts &opts, snpgpu_merge_stats *stats, snpgpu_merge_passes *passes) {
    HIP_TRY(ctx, snpgpu_enter(ctx));
    const uint64_t out_cap = 1ull << (opts.out_buffer_log2 ? opts.out_buffer_log2 : 26);
    uint64_t budget = opts.device_bytes;
    if (!budget) {
        size_t free_bytes = 0, all_bytes = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &all_bytes));
        const uint64_t reserve = free_bytes / 16 > (1ull << 30) ? free_bytes / 16 : 1ull << 30;
        budget = free_bytes > reserve ? free_bytes - reserve : 1;
    }
    MergeInput in;
    int rc = merge_read_input(ctx, paths, n_files, stats, in);
    if (rc) return rc;
    const uint64_t single = merge_single_bytes(n_files, in.total_bytes, out_cap);
    if (single <= budget) {
        *passes = snpgpu_merge_passes{1, 0, 0, single};
        rc = merge_vcf_files(ctx, paths, n_files, out_path, own_lines, own_len, out_cap, stats, &in);
        MergePlan pl;
        if (rc == SNPGPU_OK && merge_plan(n_files, stats->sites, in.total_bytes, budget, out_cap, &pl) == SNPGPU_OK) *passes = pl.p;
        return rc;
    }
    return merge_vcf_files_bounded(ctx, paths, n_files, out_path, own_lines, own_len, out_cap, budget, in, stats, passes);
}

#undef STREAM_TRY
}  // namespace

extern "C" {

int snpgpu_vcf_count_snps_files(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, uint32_t capacity, uint64_t *out_counts,
                                uint64_t *out_unusual_off, uint64_t *out_status, int32_t *out_rc) {
    if (!ctx || !out_counts || !out_status || !out_rc || (n_files && !paths) || (capacity && !out_unusual_off))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (capacity > (1u << 20)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the capacity for unusual lines is at most 2^20");
    if (!n_files) return SNPGPU_OK;
    return vcf_count_stream(ctx, paths, n_files, capacity, out_counts, out_unusual_off, out_status, out_rc);
}

int snpgpu_vcf_count_snps_file(snpgpu_ctx *ctx, const char *path, uint32_t capacity, uint64_t *out_counts, uint64_t *out_unusual_off, uint64_t *out_status) {
    if (!path) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    int32_t file_rc = SNPGPU_OK;
    const int rc = snpgpu_vcf_count_snps_files(ctx, &path, 1, capacity, out_counts, out_unusual_off, out_status, &file_rc);
    if (rc) return rc;
    return file_rc ? snpgpu_set_error(ctx, file_rc, "cannot open or read the VCF file %s", path) : SNPGPU_OK;
}

int snpgpu_merge_vcf_files(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, const char *out_path, const char *own_lines, uint32_t own_len,
                           uint32_t options, snpgpu_merge_stats *stats) {
    if (!ctx || !paths || !out_path || !stats || (own_len && !own_lines)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    if (options && (options < 12 || options > 32)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "options: 0, or 12 to 32, the log2 of the output buffer's bytes");
    if (n_files == 0 || n_files >= (1u << 24)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the merge takes 1 to 2^24 - 1 files");
    *stats = snpgpu_merge_stats{};
    stats->columns = n_files;
    stats->bad_file = stats->bad_offset = UINT64_MAX;
    try {
        return merge_vcf_files(ctx, paths, n_files, out_path, own_lines, own_len, 1ull << (options ? options : 26), stats);
    } catch (const std::exception &e) {                         // (no exception may leave through the C ABI)
        return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "merge_vcf_files: %s", e.what());
    }
}

int snpgpu_merge_plan(uint32_t n_files, uint64_t n_sites, uint64_t total_input_bytes, const snpgpu_merge_opts *opts, snpgpu_merge_passes *out) {
    if (!out || n_files == 0 || n_files >= (1u << 24)) return SNPGPU_E_ARG;
    const uint32_t log2 = opts ? opts->out_buffer_log2 : 0;
    if (log2 && (log2 < 12 || log2 > 32)) return SNPGPU_E_ARG;
    MergePlan pl;
    const int rc = merge_plan(n_files, n_sites, total_input_bytes, opts ? opts->device_bytes : 0, 1ull << (log2 ? log2 : 26), &pl);
    *out = pl.p;
    return rc;
}

int snpgpu_merge_vcf_files_opts(snpgpu_ctx *ctx, const char *const *paths, uint32_t n_files, const char *out_path, const char *own_lines, uint32_t own_len,
                                const snpgpu_merge_opts *opts, snpgpu_merge_stats *stats, snpgpu_merge_passes *passes) {
    if (!ctx || !paths || !out_path || !stats || (own_len && !own_lines)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "null argument");
    const snpgpu_merge_opts o = opts ? *opts : snpgpu_merge_opts{};
    if (o.out_buffer_log2 && (o.out_buffer_log2 < 12 || o.out_buffer_log2 > 32))
        return snpgpu_set_error(ctx, SNPGPU_E_ARG, "out_buffer_log2: 0, or 12 to 32, the log2 of the output buffer's bytes");
    if (n_files == 0 || n_files >= (1u << 24)) return snpgpu_set_error(ctx, SNPGPU_E_ARG, "the merge takes 1 to 2^24 - 1 files");
    *stats = snpgpu_merge_stats{};
    stats->columns = n_files;
    stats->bad_file = stats->bad_offset = UINT64_MAX;
    snpgpu_merge_passes mine{};
    try {
        const int rc = merge_vcf_files_planned(ctx, paths, n_files, out_path, own_lines, own_len, o, stats, &mine);
        if (passes) *passes = mine;
        return rc;
    } catch (const std::exception &e) {                         // (no exception may leave through the C ABI)
        return snpgpu_set_error(ctx, SNPGPU_E_NOMEM, "merge_vcf_files: %s", e.what());
    }
}

}  // extern "C"
