// The BGZF index and the serial host inflater (csrc/bgzf_host.hip, csrc/bgzf_core.h: the decode statements the inflate kernel
// runs too) over a directory of well-formed and malformed files, as a stand-alone program, so that it can be built with
// AddressSanitizer and UndefinedBehaviorSanitizer on the host side and an index out of bounds in the shared decode code shows
// up as a report here, on a CPU, before the same bytes go near a GPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fno-gpu-sanitize -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/probe/bgzf_host_check.hip snp_pipeline_amd/csrc/bgzf_host.hip -o check
//   ./check DIR
//
// DIR/manifest.txt has a line per case: <file> <return code of the index> <blocks before the bad header> <plain file or -> <status,status,...>
// (tests/test_bgzf_cpu.py writes it).  For a file the index takes, every block is inflated, its status compared with the
// listed one, and the text of the good blocks with the plain file at the block's plain offset; then snpgpu_bgzf_read_range is
// asked for ranges across every block boundary and at the last byte.  It uses no HIP call and needs no device.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/snpgpu.h"

static bool slurp(const std::string &path, std::vector<uint8_t> &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    out.clear();
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    FILE *mf = fopen((dir + "/manifest.txt").c_str(), "r");
    if (!mf) { fprintf(stderr, "no manifest in %s\n", argv[1]); return 2; }
    char name[256], plain_name[256], statuses[4096];
    int want_rc = 0, failures = 0, cases = 0;
    unsigned long long want_valid = 0;
    while (fscanf(mf, "%255s %d %llu %255s %4095s", name, &want_rc, &want_valid, plain_name, statuses) == 5) {
        ++cases;
        std::vector<uint8_t> data, plain;
        if (!slurp(dir + "/" + name, data)) { fprintf(stderr, "%s: cannot read\n", name); ++failures; continue; }
        const bool have_plain = strcmp(plain_name, "-") != 0;
        if (have_plain && !slurp(dir + "/" + plain_name, plain)) { fprintf(stderr, "%s: cannot read %s\n", name, plain_name); ++failures; continue; }
        // exactly the bytes of the file on the heap, so that a read one byte past them is a report
        uint8_t *exact = (uint8_t *)malloc(data.size() ? data.size() : 1);
        if (!data.empty()) memcpy(exact, data.data(), data.size());
        uint64_t n = 0;
        snpgpu_bgzf_info info;
        int rc = snpgpu_bgzf_index(exact, data.size(), nullptr, 0, &n, &info);
        if (rc != want_rc || n != want_valid) {
            fprintf(stderr, "%s: index returned %d with %llu blocks, expected %d with %llu\n", name, rc, (unsigned long long)n, want_rc, want_valid);
            ++failures;
        }
        const int probe = snpgpu_bgzf_probe((dir + "/" + name).c_str());
        const int want_probe = data.empty() || want_rc == SNPGPU_BGZF_E_NOT_GZIP ? 0 : want_rc == SNPGPU_BGZF_E_NOT_BGZF ? SNPGPU_BGZF_E_NOT_BGZF : -1000;
        if (want_probe != -1000 && probe != want_probe) { fprintf(stderr, "%s: probe returned %d, expected %d\n", name, probe, want_probe); ++failures; }
        if (want_probe == -1000 && want_valid > 0 && probe != 1) { fprintf(stderr, "%s: probe returned %d, expected 1\n", name, probe); ++failures; }
        if (rc == SNPGPU_OK) {
            std::vector<snpgpu_bgzf_block> blocks(n);
            rc = snpgpu_bgzf_index(exact, data.size(), blocks.data(), n, &n, &info);
            std::vector<unsigned> want_st;
            for (char *tok = strtok(statuses, ","); tok; tok = strtok(nullptr, ",")) if (strcmp(tok, "-") != 0) want_st.push_back((unsigned)atoi(tok));
            if (want_st.size() != n) { fprintf(stderr, "%s: %llu blocks, %zu statuses listed\n", name, (unsigned long long)n, want_st.size()); ++failures; free(exact); continue; }
            bool all_ok = true;
            for (uint64_t i = 0; i < n; ++i) {
                const snpgpu_bgzf_block &b = blocks[i];
                uint8_t *text = (uint8_t *)malloc(b.isize ? b.isize : 1);      // exactly ISIZE bytes: a write past them is a report
                const uint32_t st = snpgpu_bgzf_inflate_block_host(exact + b.coff, &b, text);
                if (st != want_st[i]) { fprintf(stderr, "%s: block %llu ended with status %u (%s), expected %u\n", name, (unsigned long long)i, st, snpgpu_bgzf_status_name(st), want_st[i]); ++failures; }
                if (st != SNPGPU_BGZF_ST_OK) all_ok = false;
                if (st == SNPGPU_BGZF_ST_OK && have_plain && b.isize && (b.poff + b.isize > plain.size() || memcmp(text, plain.data() + b.poff, b.isize) != 0)) {
                    fprintf(stderr, "%s: the text of block %llu differs\n", name, (unsigned long long)i);
                    ++failures;
                }
                free(text);
            }
            if (all_ok && have_plain) {
                std::vector<uint64_t> at{0, plain.size() ? plain.size() - 1 : 0, plain.size()};
                for (const auto &b : blocks) { at.push_back(b.poff > 5 ? b.poff - 5 : 0); at.push_back(b.poff); }
                for (uint64_t from : at) {
                    const uint64_t want_n = from + 70000 <= plain.size() ? 70000 : plain.size() - (from < plain.size() ? from : plain.size());
                    uint8_t *got = (uint8_t *)malloc(want_n ? want_n : 1);
                    uint64_t got_n = 0;
                    const int r = snpgpu_bgzf_read_range((dir + "/" + name).c_str(), from, want_n, got, &got_n);
                    if (r != SNPGPU_OK || got_n != want_n || (want_n && memcmp(got, plain.data() + (from < plain.size() ? from : 0), want_n) != 0)) {
                        fprintf(stderr, "%s: read_range at %llu returned %d with %llu bytes, expected %llu\n", name, (unsigned long long)from, r, (unsigned long long)got_n,
                                (unsigned long long)want_n);
                        ++failures;
                    }
                    free(got);
                }
            }
        }
        free(exact);
    }
    fclose(mf);
    printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
