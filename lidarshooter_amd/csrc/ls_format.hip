// ls_format.hip -- k_format_cloud, k_cloud_map_fill + k_cloud_map_scatter: the pass of ls_format_cloud (include/lidarshooter_hip.h;
// DESIGN.md 3.3.9) from a frame's points32 / ls_hit / echo records to a cloud in a driver's own record.
//
// k_format_cloud, one lane per OUTPUT record: 16 bytes of hit, two 16-byte halves of the point, the echo word -- coalesced: lane
// after lane reads record after record --, two table entries for the firing time, then the record's operation sequence
// (ls_cloud_format.h, the one ls_debug_format_record runs on the host).  The format travels by value in the kernel arguments, so the
// loop over its fields is uniform across the wave.  Output records have any size from 1 to 128 bytes and their fields any offset:
//   <false>  each lane stores its fields byte by byte to out + i * point_step;
//   <true>   a workgroup owns a tile of consecutive records (256, or 128 above 64 bytes a record: 16 KB of LDS at most), the lanes
//            write their records into the tile in LDS, and after ONE barrier the tile goes out as what it is in memory -- one
//            contiguous run that starts 16-byte aligned (256 * step and 128 * step are multiples of 16, and so is out) -- in 16-byte
//            stores, lane after lane.  Only the last tile can end off a 16-byte boundary: its last bytes go out one by one, and no
//            byte past count * step is written.
// The organized cloud is the same kernel behind an indirection: lane c serves CELL c of the V x H raster and formats record map[c],
// or the miss of that cell.  The map is made by two small launches before it: all words kCloudNoRecord, then record i stores i at
// map[hit[i].ray] when its rank -- how many of the records i-1, i-2, i-3 carry the same ray, up to the first that differs -- equals
// the layer asked for: one 32-bit store per record, so a cell claimed twice still names one whole record.  No atomics, no waiting
// between workgroups.  Every index is checked against its bound before an address is formed from it: the record against the count,
// the ray against V * H (then ring < V and column < H), the map's entry against the count.
#include "ls_kernels.h"
#include "ls_device.h"
#include "ls_cloud_format.h"

namespace ls {

namespace {

constexpr uint32_t kCloudTileBytes = 16384;   // 256 records of 64 bytes, 128 of 128

__host__ __device__ inline uint32_t cloud_tile_records(uint32_t step) { return step <= 64u ? 256u : 128u; }

struct CloudNeeds {
    uint32_t points, time;   // the format names X, Y, Z or INTENSITY / TIME
};

template <bool STAGED>
__global__ __launch_bounds__(kBlock) void k_format_cloud(ls_cloud_format fmt, const uint4 *__restrict__ points, const uint4 *__restrict__ hits,
                                                         const uint32_t *__restrict__ echo, const uint32_t *__restrict__ d_count, uint32_t n,
                                                         const float *__restrict__ col_time, const float *__restrict__ chan_time, uint32_t V,
                                                         uint32_t H, CloudNeeds needs, const uint32_t *__restrict__ map, uint32_t tile,
                                                         uint8_t *__restrict__ out)
{
    __shared__ uint4 lds[STAGED ? kCloudTileBytes / 16 : 1];
    const uint32_t count = d_count ? min(n, *d_count) : n;
    const uint32_t total = map ? V * H : count;   // output records
    const uint32_t base = blockIdx.x * tile;      // (the grid covers n records, or the cells: whole workgroups beyond the count leave)
    if (base >= total) return;
    const uint32_t step = fmt.point_step, slot = threadIdx.x, rec = base + slot;
    if (slot < tile && rec < total) {
        uint32_t i = rec;
        bool have = true;
        if (map) {
            i = map[rec];
            have = i < count;
        }
        uint32_t p8[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, h4[4] = {rec, 0u, 0u, 0u}, e = 0u;
        if (have) {
            const uint4 h = hits[i];
            h4[0] = h.x; h4[1] = h.y; h4[2] = h.z; h4[3] = h.w;
            if (points && needs.points) {
                const uint4 a = points[2 * (size_t)i], b = points[2 * (size_t)i + 1];
                p8[0] = a.x; p8[1] = a.y; p8[2] = a.z; p8[3] = a.w;
                p8[4] = b.x; p8[5] = b.y; p8[6] = b.z; p8[7] = b.w;
            }
            if (echo) e = echo[i];
        }
        float ct = 0.0f, ch = 0.0f;
        uint32_t ring, column;
        if (needs.time && cloud_split_ray(h4[0], V, H, &ring, &column)) {
            if (col_time) ct = col_time[column];
            if (chan_time) ch = chan_time[ring];
        }
        const CloudSources src = cloud_sources(p8, h4, !have, e, ct, ch, V, H);
        uint8_t *dst = STAGED ? reinterpret_cast<uint8_t *>(lds) + slot * step : out + (size_t)rec * step;
        cloud_format_record(fmt, src, dst);
    }
    if (STAGED) {
        __syncthreads();
        const uint32_t bytes = min(tile, total - base) * step, whole = bytes >> 4;
        uint8_t *run = out + (size_t)base * step;
        for (uint32_t k = threadIdx.x; k < whole; k += kBlock) reinterpret_cast<uint4 *>(run)[k] = lds[k];
        const uint32_t at = (whole << 4) + threadIdx.x;   // the last tile's end, narrowed to bytes
        if (at < bytes) run[at] = reinterpret_cast<const uint8_t *>(lds)[at];
    }
}

__global__ __launch_bounds__(kBlock) void k_cloud_map_fill(uint32_t *__restrict__ map, uint32_t cells)
{
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c < cells) map[c] = kCloudNoRecord;
}

__global__ __launch_bounds__(kBlock) void k_cloud_map_scatter(const uint4 *__restrict__ hits, const uint32_t *__restrict__ d_count, uint32_t n,
                                                              uint32_t layer, uint32_t cells, uint32_t *__restrict__ map)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t count = d_count ? min(n, *d_count) : n;
    if (i >= count) return;
    const uint32_t ray = hits[i].x;
    if (ray >= cells) return;   // not of this raster: left out
    uint32_t rank = 0;
    while (rank < 3u && rank < i && hits[i - rank - 1u].x == ray) ++rank;
    if (rank == layer) map[ray] = i;
}

}  // namespace

void launch_cloud_map(hipStream_t s, const void *hits, const uint32_t *d_count, uint32_t n, uint32_t layer, uint32_t cells, uint32_t *map)
{
    if (!cells) return;
    hipLaunchKernelGGL(k_cloud_map_fill, dim3((cells + kBlock - 1) / kBlock), dim3(kBlock), 0, s, map, cells);
    if (!n) return;
    hipLaunchKernelGGL(k_cloud_map_scatter, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, static_cast<const uint4 *>(hits), d_count, n, layer,
                       cells, map);
}

void launch_format_cloud(hipStream_t s, const ls_cloud_format &fmt, const CloudInputs &in, const uint32_t *map, void *out, int form)
{
    const uint32_t records = map ? in.V * in.H : in.n;
    if (!records) return;
    CloudNeeds needs = {0u, 0u};
    for (uint32_t k = 0; k < fmt.n_fields; ++k) {
        const uint32_t src = fmt.fields[k].source;
        if (src >= LS_FIELD_X && src <= LS_FIELD_INTENSITY) needs.points = 1u;
        if (src == LS_FIELD_TIME) needs.time = 1u;
    }
    const bool staged = form == kCloudFormStaged;
    const uint32_t tile = staged ? cloud_tile_records(fmt.point_step) : (uint32_t)kBlock;
    const dim3 grid((records + tile - 1) / tile);
    auto kernel = staged ? k_format_cloud<true> : k_format_cloud<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, fmt, static_cast<const uint4 *>(in.points32), static_cast<const uint4 *>(in.hits), in.echo,
                       in.d_count, in.n, in.col_time, in.chan_time, in.V, in.H, needs, map, tile, static_cast<uint8_t *>(out));
}

}  // namespace ls
