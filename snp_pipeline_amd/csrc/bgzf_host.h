// bgzf_host.hip: the parts of the BGZF reader that need neither a context nor the HIP runtime.
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/snpgpu.h"

// The table of a file, from a header-hopping pass over the mapped file; *map (to be munmap'ed by the caller when the return value
// is 0 and *map is not null) stays mapped for callers that go on to inflate on the host.  info is nullable.
int snpgpu_bgzf_index_file(const char *path, std::vector<snpgpu_bgzf_block> &blocks, snpgpu_bgzf_info *info, const uint8_t **map, uint64_t *map_bytes);
// what a table entry must satisfy before anything reads by it (sizes within the format's limits, header and footer inside the block)
bool snpgpu_bgzf_block_entry_ok(const snpgpu_bgzf_block &b);
