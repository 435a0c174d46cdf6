// gpu_huffman_host.h -- host-side preparation for the GPU entropy decoder (stream destuffing, table expansion, image
// descriptors) and a host emulation of the complete multi-pass algorithm, built from the same core as the kernels.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "huffman_gpu_core.h"
#include "jpeg_syntax.h"

namespace hipjpeg {

// Baseline/extended sequential frames in at most kMaxSeqScans scans (any component order inside a scan) that code every component
// exactly once; every scan with plain byte stuffing, every restart interval closed by its marker, at most 10 blocks per MCU and lookup
// tables that fit kMaxPoolWords.  Every scan is a stream of its own on the GPU (one HuffImage each).  Everything else takes the host
// entropy stage.
constexpr int kMaxSeqScans = 4;
bool gpu_entropy_eligible(const FrameInfo& f);

// MCU grid of a scan: a one-component scan has one block per MCU over the component's real blocks, any other the frame's MCU grid.
uint32_t scan_mcus_x(const FrameInfo& f, const ScanHeader& sc);
uint32_t scan_mcus_y(const FrameInfo& f, const ScanHeader& sc);
uint32_t scan_blocks_per_mcu(const FrameInfo& f, const ScanHeader& sc);

// Upper bound of the destuffed size (+ slack) for staging allocation.
inline size_t destuffed_capacity(const ScanHeader& sc) { return (((sc.data_end - sc.data_begin) + 3) & ~(size_t)3) + kStreamSlackBytes; }

// Removes byte stuffing (FF 00 -> FF) and fill bytes from the scan's entropy-coded segment; appends kStreamSlackBytes of
// 0xFF.  Returns the number of real bytes written.
size_t destuff_scan(const uint8_t* data, const ScanHeader& sc, uint8_t* out);

// Number of uint16 lookup-table entries the scan's Huffman tables expand to (first-level tables of the DC/AC tables the
// scan references + one 64-entry second-level table per 10-bit prefix that continues into longer codes); 0 = a table is
// missing or malformed (over-subscribed code, DC symbol > 15).  gpu_entropy_eligible() uses it.
size_t gpu_pool_words(const ScanHeader& sc);

// Expands the tables into `pool` (gpu_pool_words(sc) entries) and records the per-position table offsets in im->k[].tdc/tac.
// Call after fill_huff_image().
void build_gpu_pool(const ScanHeader& sc, HuffImage* im, uint16_t* pool);

// Test support (hipjpegTestPairSteps): the step a position walk takes at every 10-bit window w of AC table `ac` from every zigzag
// position z, from the table's first-level and pair entries as build_gpu_pool() lays them out and with the walks' own test
// (pair_fits): out[w * 64 + z] = bits consumed | zigzag advance << 8 | (a pair was taken) << 16 | (the window opens a long code, which
// the step leaves to the second level: nothing consumed) << 17.  False for a table the stage would refuse.
bool pair_table_steps(const HuffSpec& ac, uint32_t* out);

// Describes scan `sc` of frame `f`: every field except the pointers (stream, pool, coef, dc_diff, dc_plane), first_subseq and the
// table offsets.  Slot i of the per-component arrays (coef, dc_plane, blocks_w, comp_h/v/k0, HuffK::comp) is the scan's i-th
// component, frame component sc.comp_index[i].
void fill_huff_image(const FrameInfo& f, const ScanHeader& sc, uint32_t stream_bytes, HuffImage* im);

// Runs pass 0, the synchronisation passes, the block-count scan, the write pass and the DC integration on the host, one
// "lane" after the other, scan by scan (blocks no scan codes are left zero).  coef[c] = device-layout blocks (as entropy_decode.h).  Returns 0 on success, else the status the
// kernels would report; *sync_passes receives the number of passes until the fixpoint.  Self-checks: 4 = the cooperative walk
// disagrees with the lane walk, 5 = a block-start record disagrees with the position walk, the two forms of the lane walk
// (select_walk and decode_subsequence) disagree in end state or record, or the table classes do not reproduce the per-position
// table selection, or the first sync launch's schedule (emulate_sync_launch below) does not end in the Jacobi fixpoint's states and
// records.
// schedules (nullptr: not wanted): [0] the one-unit schedule, [1] the paired one, summed over the scans.
struct SyncScheduleCounts {
    // Subsequence decodes of the first sync launch's workgroups, halo rows included.  One unit per workgroup: pass 0 | - | correction
    // round 1 | round 2.  Two units (huff_sync_pair_kernel): phase A | phase B | round 1 | round 2.
    uint64_t phase[4];
    uint64_t tail;  // tasks left when round 2 is over: what the tail kernel's first round gets from the launch
};
int emulate_gpu_entropy(const uint8_t* data, size_t size, const FrameInfo& f, int16_t* const coef[4], int* sync_passes,
                        SyncScheduleCounts schedules[2] = nullptr);

}  // namespace hipjpeg
