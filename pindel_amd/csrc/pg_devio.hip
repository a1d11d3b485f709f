// pg_devio.hip -- the kernels of the device-buffer entries (pg_load_reference_device, pg_device_batch_upload_device,
// pg_device_batch_download_device; pindel_pg.h): what the host entries do on host threads before their copies, done where the
// caller's data already is.
//   pack reference   ASCII bases of one chromosome -> its words of the three bit planes (the device twin of pg_load_reference's pack)
//   measure reads    one pass over a batch's arrays: first bad read, longest read, largest insert size, the uniform length,
//                    seq_off[0] / seq_off[n], and the offsets rebased to 0 (the device twin of validate_and_measure)
//   store totals     close_off[n] / far_off[n] of a download from the last chunk's info, without a host value in between
// Streaming kernels, not search kernels: the default code generation (Makefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_device.h"

typedef uint32_t u32;
typedef unsigned long long u64;

#define PG_DEVIO_BLOCK 256u
#define PG_DEVIO_MAX_BLOCKS 8192u                         // grid-stride above this (a 2^31-base chromosome is 2^25 groups)

// One wavefront per group of 64 bases = two words of each plane: lane k loads base 64 g + k (a coalesced byte load, whatever
// the alignment of the caller's pointer -- a slice of a larger tensor), three ballots are the group's bits of the planes.
// Bit k of word w is base 32 w + k; A C G T in upper case are 0-3, every other byte value is N; positions at or past len (the
// tail of the last word) are N.  Writes words [0, (len + 31) / 32) of lo / hi / nn, which point at the chromosome's first word.
__global__ void __launch_bounds__(PG_DEVIO_BLOCK)
pg_devio_pack_ref_kernel(const uint8_t *s, u64 len, u32 *lo, u32 *hi, u32 *nn)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 n_words = (len + 31ull) / 32ull, n_groups = (len + 63ull) / 64ull;
    const u64 n_waves = (u64)gridDim.x * (PG_DEVIO_BLOCK / 64u);
    for (u64 g = (u64)blockIdx.x * (PG_DEVIO_BLOCK / 64u) + (threadIdx.x >> 6); g < n_groups; g += n_waves) {
        const u64 p = g * 64ull + lane;
        u32 code = 4u;
        if (p < len) {
            const uint8_t ch = s[p];
            code = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
        }
        const u64 ml = __ballot(code == 1u || code == 3u), mh = __ballot(code == 2u || code == 3u), mn = __ballot(code == 4u);
        const u64 w = 2ull * g + lane;
        if (lane < 2u && w < n_words) {
            lo[w] = (u32)(ml >> (32u * lane));
            hi[w] = (u32)(mh >> (32u * lane));
            nn[w] = (u32)(mn >> (32u * lane));
        }
    }
}

static __device__ __forceinline__ u32 wave_max_u32(u32 v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const u32 o = (u32)__shfl_xor((int)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}
static __device__ __forceinline__ u32 wave_min_u32(u32 v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const u32 o = (u32)__shfl_xor((int)v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}
static __device__ __forceinline__ int wave_max_i32(int v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const int o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}
static __device__ __forceinline__ u64 wave_min_u64(u64 v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const u32 ol = (u32)__shfl_xor((int)(u32)v, d, 64), oh = (u32)__shfl_xor((int)(u32)(v >> 32), d, 64);
        const u64 o = ((u64)oh << 32) | ol;
        v = o < v ? o : v;
    }
    return v;
}

// One thread per read i < n (and one more for the last offset).  Per read the checks of validate_and_measure (pg_api.cpp) in its
// order -- 1 seq_off not monotone, 2 longer than PG_MAX_READ_LEN, 3 chr_id out of range, 4 anchor window outside the padded
// chromosome: the first that applies is the read's code -- and the lowest bad read index wins, as in a sequential scan: one
// atomicMin per wavefront on the key (index << 8) | code.  The good reads fold their length (max and min: the batch has one
// length when they agree) and insert size (max) the same way.  off_out[i] = seq_off[i] - seq_off[0], n + 1 entries.
// *rec is initialised by the host: first_bad = PG_MEASURE_NONE, len_max = 0, len_min = ~0, isz_max = 0.
__global__ void __launch_bounds__(PG_DEVIO_BLOCK)
pg_devio_measure_kernel(const u64 *seq_off, const int32_t *pos, const int16_t *isz, const int32_t *chr, u32 n, const u32 *chr_size,
                        int32_t n_chr, u32 spacer, u64 *off_out, PgReadMeasure *rec)
{
    const u64 i = (u64)blockIdx.x * PG_DEVIO_BLOCK + threadIdx.x;
    const u64 base0 = seq_off[0];
    u64 key = PG_MEASURE_NONE;
    u32 len_max = 0u, len_min = 0xffffffffu;
    int isz_max = 0;
    if (i < n) {
        const u64 o0 = seq_off[i], o1 = seq_off[i + 1];
        off_out[i] = o0 - base0;
        u32 code = 0u;
        if (o1 < o0) code = 1u;
        const u64 len = o1 - o0;
        if (!code && len > (u64)PG_MAX_READ_LEN) code = 2u;
        const int c = chr[i];
        if (!code && (c < 0 || c >= n_chr)) code = 3u;
        const long long is = isz[i];
        if (!code) {
            const long long apos = (long long)pos[i] + (long long)spacer, reach = 2ll * (is > 0 ? is : 0ll) + 2ll;
            if (apos - reach < 0 || apos + reach > (long long)chr_size[c]) code = 4u;
        }
        if (code) key = (i << 8) | code;
        else {
            len_max = len_min = (u32)len;
            isz_max = (int)is;
        }
    } else if (i == n) {
        const u64 on = seq_off[n];
        off_out[n] = on - base0;
        rec->off0 = base0;
        rec->offn = on;
    }
    key = wave_min_u64(key);
    len_max = wave_max_u32(len_max);
    len_min = wave_min_u32(len_min);
    isz_max = wave_max_i32(isz_max);
    if ((threadIdx.x & 63u) == 0u) {
        if (key != PG_MEASURE_NONE) atomicMin(&rec->first_bad, key);
        if (len_min != 0xffffffffu) {                     // (a wavefront with a good read)
            atomicMax(&rec->len_max, len_max);
            atomicMin(&rec->len_min, len_min);
        }
        if (isz_max > 0) atomicMax(&rec->isz_max, isz_max);
    }
}

// info: the 8 values pg_deliver_scan left for the batch's LAST chunk {close base, far base, close runs, far runs, ...}
__global__ void pg_devio_store_totals_kernel(const u64 *info, u64 *close_end, u64 *far_end)
{
    if (threadIdx.x == 0u) {
        *close_end = info[0] + info[2];
        *far_end = info[1] + info[3];
    }
}

extern "C" int pg_devio_pack_reference(const uint8_t *d_seq, unsigned long long len, uint32_t *lo, uint32_t *hi, uint32_t *nn, void *stream)
{
    if (!len) return 0;
    const u64 n_groups = (len + 63ull) / 64ull, per = PG_DEVIO_BLOCK / 64u;
    const u32 blocks = (u32)((n_groups + per - 1ull) / per < PG_DEVIO_MAX_BLOCKS ? (n_groups + per - 1ull) / per : PG_DEVIO_MAX_BLOCKS);
    pg_devio_pack_ref_kernel<<<blocks, PG_DEVIO_BLOCK, 0, (hipStream_t)stream>>>(d_seq, len, lo, hi, nn);
    return (int)hipGetLastError();
}

extern "C" int pg_devio_measure_reads(const unsigned long long *seq_off, const int32_t *pos, const int16_t *isz, const int32_t *chr,
                                      uint32_t n, const uint32_t *chr_size, int32_t n_chr, uint32_t spacer,
                                      unsigned long long *off_out, struct PgReadMeasure *rec, void *stream)
{
    if (!n) return 0;
    const u32 blocks = (u32)(((u64)n + 1ull + PG_DEVIO_BLOCK - 1ull) / PG_DEVIO_BLOCK);
    pg_devio_measure_kernel<<<blocks, PG_DEVIO_BLOCK, 0, (hipStream_t)stream>>>(seq_off, pos, isz, chr, n, chr_size, n_chr, spacer, off_out, rec);
    return (int)hipGetLastError();
}

extern "C" int pg_devio_store_totals(const unsigned long long *info, unsigned long long *close_end, unsigned long long *far_end, void *stream)
{
    pg_devio_store_totals_kernel<<<1, 64, 0, (hipStream_t)stream>>>(info, close_end, far_end);
    return (int)hipGetLastError();
}
