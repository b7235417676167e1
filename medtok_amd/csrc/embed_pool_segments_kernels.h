// Segment pooling: one row per (batch row, segment) from the stored token table -- MedTokEmbedding.pooled_segments, the visit-level input
// of an EHR transformer (the reference's patientEncoder_old runs over [B, max_visit_num, dim] visit embeddings, EHRModel_token.py:249-292).
// Included by medtok_vq.hip behind embed_kernels.h, ema_kernels.h and embed_grad_kernels.h.
//
//   out[b, v] = ( sum over the unpadded p with segment_id[b, p] == v of n(row(b, p)) ) / count[b, v]
//
// is embed_pool_partial_kernel's bag pooling with one indirection in front: a bag is a LIST of positions.  The lists come from the scan
// and the stable radix sort of the EMA statistics, planned as the codebook gradient plans its rows (embed_grad_kernels.h):
//   embed_code_grad_zero_kernel        the histogram's zeros (a kernel, not a memset node)
//   embed_pool_segments_keys_kernel    one thread per position: key = b * V + g for an unpadded position with 0 <= g < V, else B * V
//                                      (dead: sorts behind every bag); payload = the flat position; integer histogram of the live keys;
//                                      bit MEDTOK_EMBED_BAD_SEGMENT_BIT of *status for an unpadded g outside [0, V).  A padded position
//                                      reads no segment id; no id forms an address before it has been checked; the products are 64-bit.
//   scan_kernel                        offsets[B * V + 1]
//   embed_code_grad_plan_kernel<16>    chunks[bag] for the bags longer than one chunk, scanned into first_chunk[]
//   radix_count / radix_scatter        the stable sort by key: bag g's positions are sorted[offsets[g] .. offsets[g + 1]), ascending
//   embed_pool_partial_kernel<.., true>  blocks [0, B * V): a bag of at most one chunk is finished there; blocks behind: the chunks of the
//                                      longer bags (at most Q = ceil(2 * B * L / 16): a bag of len > 16 has ceil(len / 16) < 2 len / 16)
//   embed_pool_finish_kernel           the bags with several chunks: chunk sums in chunk order from +0, the division, the counts
// Every step is a kernel launch and nothing is read back: the call records into a HIP graph.  No float atomics; the order is fixed by
// (index, segment_id, pad, tables) alone.
#pragma once

__global__ __launch_bounds__(256) void embed_pool_segments_keys_kernel(const uint8_t *__restrict__ pad, const int64_t *__restrict__ segment_id,
                                                                       long n, long len, long n_segments, uint32_t dead,
                                                                       uint32_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                                       int *__restrict__ counts, int *status)
{
    const long pos = (long)blockIdx.x * 256 + threadIdx.x;
    if (pos >= n) return;
    uint32_t key = dead;
    if (!(pad && pad[pos] != 0)) {
        const long g = segment_id[pos];
        if (g >= 0 && g < n_segments) key = (uint32_t)((pos / len) * n_segments + g);     // < B * V < 2^31 (checked on the host)
        else if (status) atomicOr(status, 1 << MEDTOK_EMBED_BAD_SEGMENT_BIT);
    }
    keys[pos] = key;
    vals[pos] = (uint32_t)pos;                                    // n < 2^31 (checked on the host)
    if (key != dead) atomicAdd(&counts[key], 1);                  // (integer: exact in any order)
}
