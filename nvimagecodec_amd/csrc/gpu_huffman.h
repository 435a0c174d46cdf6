// gpu_huffman.h -- host-callable launchers of the GPU entropy kernels (gpu_huffman.hip); stream = hipStream_t as void*.
#pragma once
#include <cstdint>

#include "huffman_gpu_core.h"

namespace hipjpeg {

// sync/write kernels: `first` = first subsequence (inside the image) the workgroup owns (it owns kHuffOwn of them); dc kernel: `first` = component index
struct HuffUnit {
    uint32_t image;  // index into HuffImage[]
    uint32_t first;
};

// Byte-stuffing removal (count + compact): chunk_units[i] = {image, chunk index inside the image}; drops = one uint32 per chunk.
// Writes HuffImage::stream contents and total_bits / num_subseq / stream_words.
// count_on_device = false: `drops` already holds the per-chunk counts (from the host's marker walk)
// counters: 64 words the compact kernel clears (the stage's convergence counters)
// Zero-copy input: copies the scans of the images whose HuffImage::raw_src is set from the caller's pinned host memory to HuffImage::raw
// (same chunk units as the destuff kernels; images without raw_src are skipped).
int launch_gather_raw(const HuffImage* images, const HuffUnit* chunk_units, int nchunks, void* stream);
int launch_destuff(HuffImage* images, const HuffUnit* chunk_units, int nchunks, uint32_t* drops, bool count_on_device, unsigned int* counters,
                   void* stream);

// pool_bytes = dynamic LDS for the lookup tables: 2 * the largest HuffImage::pool_words of the batch
// units[i].first = first owned subsequence of workgroup i, a multiple of kHuffOwn; incoming = one uint64 per unit
// max_rounds / tail_tasks / tail_count: after max_rounds correction rounds the workgroup hands what is left (tail_tasks:
// kTailTaskBytes per unit, tail_count: one uint32 per unit) to the tail kernel, launched right behind it; tail_count == nullptr:
// the workgroup iterates to its fixpoint itself.  The tail kernel enters a group with the state that lies in front of it at that
// moment, not with pass 0's guess (incoming[] then holds the state that was used): most corrections across group borders are
// made there already, and the ripple launch finds little.
// first_pass == 0: a ripple launch (corrections across group borders), pass_id = its number (1, 2, ...): HuffImage::moved_pass
// receives it for every image in which a group's own last end state still changed.  HuffImage::gave_up is set for images with a
// group that exceeded its round budget (periodic streams); such images are skipped by later ripple launches.
// records: block-start records of the synchronisation decodes (huffman_gpu_core.h), kRecShorts uint16 per subsequence, batch-wide
// like the end states (index HuffImage::first_subseq + subsequence).  Every correction decode of an owned subsequence records
// where its blocks start and writes its mark (not in streams with restart intervals), and so do the first launch's decodes from a
// neighbour's end state (phase B of the paired schedule); decodes from the assumed state record nothing.
// pairs (first_pass only): the first launch's workgroups take two consecutive units of an image each -- pairs[i] = index of the first
// unit, bit 31 set where the next unit belongs to the same image and is taken along (huff_pair_entry); what the launch leaves is per
// unit all the same.
constexpr uint32_t huff_pair_entry(uint32_t first_unit, bool with_next) { return first_unit | (with_next ? 0x80000000u : 0u); }
int launch_huff_sync(HuffImage* images, const HuffUnit* units, int nunits, const uint32_t* pairs, int npairs, unsigned long long* states,
                     unsigned long long* incoming, unsigned int* changed, int first_pass, int max_rounds, uint16_t* tail_tasks, uint32_t* tail_count,
                     uint16_t* records, unsigned pool_bytes, void* stream, unsigned pass_id = 0);
// Write pass: the block positions over the sync units, then the block kernel over block_units ({image, first MCU}, kHuffMcusPerWg
// MCUs each).  One kernel numbers the blocks (the block in progress where every subsequence begins: first_block, written for the
// subsequences that are walked; HuffImage::decoded_blocks and the "stream ends before the last block" status) and puts every usable
// record into HuffImage::block_pos; the position kernel behind it walks only the other subsequences: overflowed records, images with
// restart intervals; every subsequence when records == nullptr (HIPJPEG_POSITION_PASS=1).  walkers: one uint32 per sync unit,
// between the two.  Every image with a scan to decode needs a sync unit at subsequence 0, also when its stream is empty.
// group_sums: four int32 per block unit -- the sums of the DC differences of its MCUs, per component (what the DC pass needs
// from the groups in front of a group).
// dc_only: the pixel kernels decode the blocks themselves (decode_kernels.hip FUSED builds); only the DC differences are read here.
int launch_huff_write(HuffImage* images, const HuffUnit* sync_units, int nsync_units, const HuffUnit* block_units, int nblock_units,
                      const unsigned long long* states, uint32_t* first_block, const uint16_t* records, uint32_t* walkers,
                      int32_t* group_sums, unsigned pool_bytes, void* stream, bool dc_only = false);
// DC differences -> DC planes.  Images without restart intervals: one workgroup per block unit (its base = the sums of the
// units in front of it); images with restart intervals: one workgroup per (image, component) in rst_units.
// verdicts (nullptr: none): what the host reads of the stage, written by the first of these kernels -- kHuffVerdictCounters words of
// `counters` (the sync launches' convergence counters), then huff_verdict() of every image that has a block unit: what the converged
// path of resolve() needs, the status and gave_up (moved_pass matters only where the launches did not converge, and there the host
// fetches the descriptors).  Memory the device
// can store to: the host's pinned memory where it is mapped.
constexpr int kHuffVerdictCounters = 8;
constexpr uint32_t huff_verdict(uint32_t status, uint32_t gave_up) { return (status & 0xFFu) | (gave_up ? 0x100u : 0u); }
constexpr uint32_t huff_verdict_status(uint32_t v) { return v & 0xFFu; }
constexpr bool huff_verdict_gave_up(uint32_t v) { return (v & 0x100u) != 0; }
int launch_huff_dc(const HuffImage* images, const HuffUnit* rst_units, int nrst_units, const HuffUnit* block_units, int nblock_units,
                   const int32_t* group_sums, const unsigned int* counters, unsigned int* verdicts, void* stream);

}  // namespace hipjpeg
