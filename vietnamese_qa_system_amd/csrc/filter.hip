// Tile compaction of a filtered search (vqa_index_search_filtered, capi.hip), gfx950 only.
//
// The caller's row bitmap (bit p & 31 of word p >> 5 allows row position p) -> the ascending list of the 256-row tiles that hold at
// least one allowed row, and its length, in the handle's workspace.  The filtered scan (score_topk.hip MODE 3) then reads only those
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
