// Tile compaction of a filtered search (vqa_index_search_filtered, capi.hip), gfx950 only.
//
// The caller's row bitmap (bit p & 31 of word p >> 5 allows row position p) -> the ascending list of the 256-row tiles that hold at
// least one allowed row, and its length, in the handle's workspace (one bitmap per query: the union over a query tile's bitmaps, below).  The filtered scan (score_topk.hip MODE 3) then reads only those
// tiles.  A tile is its 8 words; the words of the last tile are read only up to ceil(n / 32) and the bits of the last word past n are
// ignored.  Two launches over chunks of kChunk tiles: (1) allowed tiles per chunk, (2) every chunk's offset = the sum of the counts
// before it, then its tiles in order.  At 10M rows that is 1.25 MB read twice by a few dozen workgroups; nothing reaches the host.
#include "vqa_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 4;  // consecutive tiles per thread
constexpr int kChunk = kThreads * kPerThread;

// bit i: tile (first + i) holds an allowed row (tiles past the shard read nothing)
__device__ __forceinline__ unsigned tile_bits(const uint32_t* __restrict__ allow, long long n, long long first) {
    const long long nwords = (n + 31) / 32;
    const long long tiles = (n + 255) / 256;
    const uint32_t last_mask = (n & 31) ? (1u << (n & 31)) - 1u : 0xFFFFFFFFu;
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        const long long t = first + i;
        if (t >= tiles) break;
        uint32_t any = 0;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const long long wi = t * 8 + w;
            if (wi < nwords) any |= allow[wi] & (wi == nwords - 1 ? last_mask : 0xFFFFFFFFu);
        }
        bits |= (any != 0u) << i;
    }
    return bits;
}

// exclusive prefix sum of v over the block (and the block total)
__device__ __forceinline__ int block_scan(int v, int* sh, int& total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const int o = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += o;
        __syncthreads();
    }
    total = sh[kThreads - 1];
    return sh[tid] - v;
}

__global__ __launch_bounds__(kThreads) void filter_count_kernel(const uint32_t* __restrict__ allow, long long n, int* __restrict__ chunk_cnt) {
    __shared__ int sh[kThreads];
    const long long first = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kPerThread;
    int total = 0;
    (void)block_scan(__builtin_popcount(tile_bits(allow, n, first)), sh, total);
    if (threadIdx.x == 0) chunk_cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void filter_list_kernel(const uint32_t* __restrict__ allow, long long n, const int* __restrict__ chunk_cnt,
                                                               int* __restrict__ tiles, int* __restrict__ count) {
    __shared__ int sh[kThreads];
    // this chunk's offset: the allowed tiles of the chunks before it
    int before = 0;
    for (int c = threadIdx.x; c < (int)blockIdx.x; c += kThreads) before += chunk_cnt[c];
    int offset = 0;
    (void)block_scan(before, sh, offset);
    __syncthreads();
    const long long first = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kPerThread;
    unsigned bits = tile_bits(allow, n, first);
    int total = 0;
    int at = offset + block_scan(__builtin_popcount(bits), sh, total);
    while (bits) {
        const int i = __builtin_ctz(bits);
        bits &= bits - 1;
        tiles[at++] = (int)(first + i);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *count = offset + total;
}

// ---- one bitmap per query (vqa_index_search_filtered_multi): the list of one query tile is the union of its queries' bitmaps.
// Every block first reads the tile's nq entries of query_filter and keeps the distinct bitmaps they name in LDS, so that a bitmap
// shared by many queries is read once (bytes read: bitmaps used x n / 8, twice); an entry of -1 lists every tile.

// normalised entry of query t: a bitmap index in [0, F), kFilterAll, or kFilterNone (any other value, and queries past nq)
__device__ __forceinline__ int filter_entry(const int* __restrict__ qf, int t, int nq, int F) {
    if (t >= nq) return kFilterNone;
    const int e = qf[t];
    return e >= 0 && e < F ? e : e == -1 ? kFilterAll : kFilterNone;
}

struct UsedFilters {
    int n;     // distinct bitmaps, in sh_list[0, n)
    bool all;  // some query searches every row
};

// the distinct bitmap indices of the tile's queries -> sh_list (order of first use); sh_e: every query's normalised entry
__device__ __forceinline__ UsedFilters used_filters(const int* __restrict__ qf, int nq, int F, int* sh_e, int* sh_list, int* sh) {
    static_assert(kThreads == VQA_QUERY_TILE, "one thread per query of the tile");
    const int t = threadIdx.x;
    const int e = filter_entry(qf, t, nq, F);
    sh_e[t] = e;
    __syncthreads();
    bool first = e >= 0;
    for (int u = 0; u < t && first; ++u) first = sh_e[u] != e;  // broadcast reads
    UsedFilters r;
    const int at = block_scan(first ? 1 : 0, sh, r.n);
    if (first) sh_list[at] = e;
    r.all = __syncthreads_or(e == kFilterAll) != 0;  // (also the barrier sh_list needs)
    return r;
}

// bit i: tile (first + i) holds a row some used bitmap allows
__device__ __forceinline__ unsigned tile_bits_multi(const uint32_t* __restrict__ allow, long long n, long long first, const int* sh_list,
                                                    UsedFilters u) {
    const long long tiles = (n + 255) / 256;
    if (u.all) {
        const long long left = tiles - first;
        return left <= 0 ? 0u : left >= kPerThread ? (1u << kPerThread) - 1u : (1u << left) - 1u;
    }
    const long long nwords = (n + 31) / 32;
    unsigned bits = 0;
    for (int i = 0; i < u.n; ++i) bits |= tile_bits(allow + (size_t)sh_list[i] * nwords, n, first);
    return bits;
}

__global__ __launch_bounds__(kThreads) void filter_multi_count_kernel(const uint32_t* __restrict__ allow, long long n, const int* __restrict__ qf,
                                                                      int nq, int F, int* __restrict__ chunk_cnt) {
    __shared__ int sh[kThreads], sh_e[kThreads], sh_list[kThreads];
    const UsedFilters u = used_filters(qf, nq, F, sh_e, sh_list, sh);
    const long long first = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kPerThread;
    int total = 0;
    (void)block_scan(__builtin_popcount(tile_bits_multi(allow, n, first, sh_list, u)), sh, total);
    if (threadIdx.x == 0) chunk_cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void filter_multi_list_kernel(const uint32_t* __restrict__ allow, long long n, const int* __restrict__ qf,
                                                                     int nq, int F, const int* __restrict__ chunk_cnt, int* __restrict__ tiles,
                                                                     int* __restrict__ count, int* __restrict__ qmap) {
    __shared__ int sh[kThreads], sh_e[kThreads], sh_list[kThreads];
    const UsedFilters u = used_filters(qf, nq, F, sh_e, sh_list, sh);
    if (blockIdx.x == 0) {
        // the scan's query map: each query's entry, and per 16-query group the entry all of its live queries share (or kFilterMixed)
        qmap[threadIdx.x] = sh_e[threadIdx.x];
        if (threadIdx.x < VQA_QUERY_TILE / 16) {
            int common = kFilterNone;
            for (int i = 0; i < 16; ++i) {
                const int q = (int)threadIdx.x * 16 + i;
                if (q >= nq) break;
                if (i == 0) common = sh_e[q];
                else if (sh_e[q] != common) common = kFilterMixed;
            }
            qmap[VQA_QUERY_TILE + threadIdx.x] = common;
        }
    }
    int before = 0;
    for (int c = threadIdx.x; c < (int)blockIdx.x; c += kThreads) before += chunk_cnt[c];
    int offset = 0;
    (void)block_scan(before, sh, offset);
    __syncthreads();
    const long long first = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kPerThread;
    unsigned bits = tile_bits_multi(allow, n, first, sh_list, u);
    int total = 0;
    int at = offset + block_scan(__builtin_popcount(bits), sh, total);
    while (bits) {
        const int i = __builtin_ctz(bits);
        bits &= bits - 1;
        tiles[at++] = (int)(first + i);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *count = offset + total;
}

}  // namespace

int vqa_filter_chunks(int64_t n) { return (int)(((n + 255) / 256 + kChunk - 1) / kChunk); }

int vqa_launch_filter_tiles(const uint32_t* allow, int64_t n, int* tiles, int* count, int* chunk_cnt, hipStream_t stream) {
    VQA_REQUIRE(allow && tiles && count && chunk_cnt && n > 0, "filter_tiles: bad arguments");
    const int chunks = vqa_filter_chunks(n);
    hipLaunchKernelGGL(filter_count_kernel, dim3(chunks), dim3(kThreads), 0, stream, allow, (long long)n, chunk_cnt);
    VQA_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(filter_list_kernel, dim3(chunks), dim3(kThreads), 0, stream, allow, (long long)n, chunk_cnt, tiles, count);
    VQA_HIP_CHECK(hipGetLastError());
    return VQA_OK;
}

int vqa_launch_filter_tiles_multi(const uint32_t* allow, int64_t n, const int* query_filter, int nq, int F, int* tiles, int* count,
                                  int* chunk_cnt, int* qmap, hipStream_t stream) {
    VQA_REQUIRE(allow && query_filter && tiles && count && chunk_cnt && qmap && n > 0 && F >= 1 && nq >= 1 && nq <= VQA_QUERY_TILE,
                "filter_tiles_multi: bad arguments");
    const int chunks = vqa_filter_chunks(n);
    hipLaunchKernelGGL(filter_multi_count_kernel, dim3(chunks), dim3(kThreads), 0, stream, allow, (long long)n, query_filter, nq, F, chunk_cnt);
    VQA_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(filter_multi_list_kernel, dim3(chunks), dim3(kThreads), 0, stream, allow, (long long)n, query_filter, nq, F, chunk_cnt,
                       tiles, count, qmap);
    VQA_HIP_CHECK(hipGetLastError());
    return VQA_OK;
}
