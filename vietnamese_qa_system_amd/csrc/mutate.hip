// In-place removal of rows from an index shard (vqa_index_remove_rows, capi.hip), gfx950 only.  A removal is a fixed number of launches
// however scattered its rows are: move (every surviving row of the tail into a hole), clear (the vacated tail), and the re-cut of the dirty
// tiles' sketch (convert.hip vqa_launch_tile_scales_list / vqa_launch_sketch_rows_list: the quantiser of set_rows, over a tile list).
// All of them move 16-byte units; nothing here computes a value.
#include "vqa_common.h"

namespace {

int grid_for(long long total) {
    const long long b = (total + 255) / 256;
    return (int)(b < 65536 ? (b > 0 ? b : 1) : 65536);
}

// one thread per 16-byte unit of a moved row: the tiled rows, the row-major copy (the same row_units units per row: d_pad elements of the
// storage type either way), and the id with unit 0.  Sources (surviving rows >= n') and destinations (removed rows < n') are disjoint sets.
__global__ __launch_bounds__(256) void move_rows_kernel(const long long* __restrict__ src, const long long* __restrict__ dst, long long pairs,
                                                        uint4* __restrict__ rows, int row_units, uint4* __restrict__ rows_rm,
                                                        long long* __restrict__ ids) {
    const int KT = row_units >> 2;
    const long long total = pairs * row_units;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long p = i / row_units;
        const int u = (int)(i - p * row_units);
        const long long s = src[p], d = dst[p];
        rows[vqa_tiled_unit(d, u >> 2, u & 3, KT)] = rows[vqa_tiled_unit(s, u >> 2, u & 3, KT)];
        if (rows_rm) rows_rm[(size_t)d * row_units + u] = rows_rm[(size_t)s * row_units + u];
        if (ids && u == 0) ids[d] = ids[s];
    }
}

// rows [first, first + count) as create leaves them: zero rows, row-major copy, int8 codes (units8 units per row) and beta; id -1
__global__ __launch_bounds__(256) void clear_rows_kernel(long long first, long long count, uint4* __restrict__ rows, int row_units,
                                                         uint4* __restrict__ rows_rm, uint4* __restrict__ rows8, int units8,
                                                         float* __restrict__ beta, long long* __restrict__ ids) {
    const int width = row_units > units8 ? row_units : units8;
    const long long total = count * width;
    const uint4 z = {0u, 0u, 0u, 0u};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long ri = i / width;
        const int u = (int)(i - ri * width);
        const long long row = first + ri;
        if (u < row_units) {
            rows[vqa_tiled_unit(row, u >> 2, u & 3, row_units >> 2)] = z;
            if (rows_rm) rows_rm[(size_t)row * row_units + u] = z;
        }
        if (rows8 && u < units8) rows8[vqa_tiled_unit(row, u >> 2, u & 3, units8 >> 2)] = z;
        if (u == 0) {
            if (beta) beta[row] = 0.f;
            if (ids) ids[row] = -1;
        }
    }
}

// host-mapped pinned words -> device memory, read by the kernel over the bus (the removal's lists: a DMA engine's first copy in a process
// costs milliseconds of setup inside hipMemcpyAsync, a kernel read of a few KB does not)
__global__ __launch_bounds__(256) void stage_words_kernel(const long long* __restrict__ mapped, long long words, long long* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (long long)gridDim.x * blockDim.x) out[i] = mapped[i];
}

}  // namespace

int vqa_launch_stage_words(const int64_t* mapped, int64_t words, int64_t* out, hipStream_t stream) {
    if (words == 0) return VQA_OK;
    VQA_REQUIRE(mapped && out, "stage_words: bad arguments");
    hipLaunchKernelGGL(stage_words_kernel, dim3(grid_for(words)), dim3(256), 0, stream, reinterpret_cast<const long long*>(mapped), (long long)words,
                       reinterpret_cast<long long*>(out));
    VQA_HIP_CHECK(hipGetLastError());
    return VQA_OK;
}

int vqa_launch_move_rows(const int64_t* src, const int64_t* dst, int64_t pairs, void* rows, int32_t row_units, void* rows_rm, int64_t* ids,
                         hipStream_t stream) {
    if (pairs == 0) return VQA_OK;
    VQA_REQUIRE(src && dst && rows && row_units > 0 && row_units % 4 == 0, "move_rows: bad arguments");
    hipLaunchKernelGGL(move_rows_kernel, dim3(grid_for(pairs * row_units)), dim3(256), 0, stream, reinterpret_cast<const long long*>(src),
                       reinterpret_cast<const long long*>(dst), (long long)pairs, reinterpret_cast<uint4*>(rows), row_units,
                       reinterpret_cast<uint4*>(rows_rm), reinterpret_cast<long long*>(ids));
    VQA_HIP_CHECK(hipGetLastError());
    return VQA_OK;
}

int vqa_launch_clear_rows(int64_t first, int64_t count, void* rows, int32_t row_units, void* rows_rm, void* rows8, int32_t units8, float* beta,
                          int64_t* ids, hipStream_t stream) {
    if (count == 0) return VQA_OK;
    VQA_REQUIRE(rows && row_units > 0 && row_units % 4 == 0 && (!rows8 || (units8 > 0 && units8 % 4 == 0)), "clear_rows: bad arguments");
    const int width = row_units > units8 ? row_units : units8;
    hipLaunchKernelGGL(clear_rows_kernel, dim3(grid_for(count * width)), dim3(256), 0, stream, (long long)first, (long long)count,
                       reinterpret_cast<uint4*>(rows), row_units, reinterpret_cast<uint4*>(rows_rm), reinterpret_cast<uint4*>(rows8),
                       rows8 ? units8 : 0, beta, reinterpret_cast<long long*>(ids));
    VQA_HIP_CHECK(hipGetLastError());
    return VQA_OK;
}
