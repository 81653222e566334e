// Microbenchmark: the two forms of k_format_cloud (lidarshooter_amd/csrc/ls_format.hip) against each other and against a
// device-to-device copy of the bytes they move -- which one ls_format_cloud ships is decided by this measurement (EXPERIMENTS.md).
//   naive   one lane per record, fields stored byte by byte to out + i * step
//   staged  records written into a tile in LDS, the tile streamed out in 16-byte stores
//   floor   hipMemcpyAsync of (48 + step) bytes per record: the 16-byte hit and the 32-byte point in, the record out
// 524 288 synthetic records (a 128 x 4096 raster, every ray a hit, ascending ray index as a frame emits them) at steps 22, 32 and 48,
// unorganized and organized (the two map launches included).  Per shape: `rounds` rounds, the three variants alternating inside a
// round, `reps` launches between two hipEvents each; median and min..max of the per-launch time over the rounds.  Both forms must
// give the same bytes as the host run of the record's sequence (ls_cloud_format.h), or the tool fails.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -I lidarshooter_amd/csrc \
//              -o tools/micro/format_forms tools/micro/format_forms.hip
#include "ls_format.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(call)                                                                              \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                      \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

static ls_cloud_format make_format(uint32_t step, bool organized)
{
    ls_cloud_format f;
    std::memset(&f, 0, sizeof(f));
    f.point_step = step;
    f.flags = organized ? LS_CLOUD_ORGANIZED : 0u;
    auto add = [&f](uint8_t source, uint8_t datatype, uint16_t offset, float scale = 1.0f) {
        ls_cloud_field &fd = f.fields[f.n_fields++];
        fd.source = source; fd.datatype = datatype; fd.offset = offset; fd.scale = scale; fd.bias = 0.0f;
    };
    if (step == 22) {          // Velodyne XYZIRT
        add(LS_FIELD_X, 7, 0); add(LS_FIELD_Y, 7, 4); add(LS_FIELD_Z, 7, 8); add(LS_FIELD_INTENSITY, 7, 12); add(LS_FIELD_RING, 4, 16);
        add(LS_FIELD_TIME, 7, 18);
    } else if (step == 32) {   // the reference's XYZIR
        add(LS_FIELD_X, 7, 0); add(LS_FIELD_Y, 7, 4); add(LS_FIELD_Z, 7, 8); add(LS_FIELD_INTENSITY, 7, 16); add(LS_FIELD_RING, 4, 20);
    } else {                   // Ouster-like, 48 bytes
        add(LS_FIELD_X, 7, 0); add(LS_FIELD_Y, 7, 4); add(LS_FIELD_Z, 7, 8); add(LS_FIELD_INTENSITY, 7, 16); add(LS_FIELD_TIME, 6, 20, 1e9f);
        add(LS_FIELD_RING, 2, 24); add(LS_FIELD_GEOM, 4, 26); add(LS_FIELD_RANGE, 6, 28, 1000.0f); add(LS_FIELD_RAY, 6, 32);
        add(LS_FIELD_RANGE, 8, 40);
    }
    return f;
}

int main(int argc, char **argv)
{
    const uint32_t V = 128, H = 4096, n = V * H;
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 9, reps = argc > 2 ? std::atoi(argv[2]) : 50;
    std::vector<uint32_t> points((size_t)n * 8), hits((size_t)n * 4);
    std::vector<float> col(H), chan(V);
    uint32_t x = 12345u;
    auto next = [&x]() { x = x * 1664525u + 1013904223u; return x; };
    for (uint32_t i = 0; i < n; ++i) {
        for (int k = 0; k < 8; ++k) {
            const float v = (float)(next() >> 8) * (1.0f / 16777216.0f) * 80.0f - 40.0f;
            std::memcpy(&points[(size_t)i * 8 + k], &v, 4);
        }
        const float t = 0.5f + (float)(next() >> 8) * (1.0f / 16777216.0f) * 100.0f;
        hits[(size_t)i * 4] = i;
        hits[(size_t)i * 4 + 1] = next() % 7u;
        hits[(size_t)i * 4 + 2] = next() % 100000u;
        std::memcpy(&hits[(size_t)i * 4 + 3], &t, 4);
    }
    for (uint32_t h = 0; h < H; ++h) col[h] = (float)(0.1 * h / H);
    for (uint32_t v = 0; v < V; ++v) chan[v] = (float)(1.5e-6 * v);
    void *d_points, *d_hits, *d_out[2], *d_src, *d_dst;
    float *d_col, *d_chan;
    uint32_t *d_map;
    const size_t out_cap = (size_t)n * 48 + 64, copy_cap = (size_t)n * 96;
    CHECK(hipMalloc(&d_points, (size_t)n * 32));
    CHECK(hipMalloc(&d_hits, (size_t)n * 16));
    CHECK(hipMalloc(&d_out[0], out_cap));
    CHECK(hipMalloc(&d_out[1], out_cap));
    CHECK(hipMalloc(&d_src, copy_cap));
    CHECK(hipMalloc(&d_dst, copy_cap));
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_col), H * 4));
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_chan), V * 4));
    CHECK(hipMalloc(reinterpret_cast<void **>(&d_map), (size_t)n * 4));
    CHECK(hipMemcpy(d_points, points.data(), (size_t)n * 32, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_hits, hits.data(), (size_t)n * 16, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_col, col.data(), H * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_chan, chan.data(), V * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_src, 1, copy_cap));
    hipStream_t s;
    hipEvent_t e0, e1;
    CHECK(hipStreamCreate(&s));
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const ls::CloudInputs in = {d_points, d_hits, nullptr, nullptr, n, d_col, d_chan, V, H};
    std::printf("{\"records\": %u, \"rounds\": %d, \"reps\": %d, \"shapes\": [\n", n, rounds, reps);
    const uint32_t steps[3] = {22, 32, 48};
    bool first = true;
    for (int organized = 0; organized < 2; ++organized)
        for (uint32_t step : steps) {
            const ls_cloud_format fmt = make_format(step, organized != 0);
            const size_t bytes = (size_t)n * step;
            auto run = [&](int variant) {   // 0 naive, 1 staged, 2 the copy
                if (variant == 2) {
                    (void)hipMemcpyAsync(d_dst, d_src, (size_t)n * (48 + step), hipMemcpyDeviceToDevice, s);
                    return;
                }
                if (organized) ls::launch_cloud_map(s, d_hits, nullptr, n, 0, n, d_map);
                ls::launch_format_cloud(s, fmt, in, organized ? d_map : nullptr, d_out[variant], variant);
            };
            // the same bytes from both forms, and the host's
            CHECK(hipMemset(d_out[0], 0xAB, out_cap));
            CHECK(hipMemset(d_out[1], 0xAB, out_cap));
            run(0);
            run(1);
            CHECK(hipStreamSynchronize(s));
            CHECK(hipGetLastError());
            std::vector<uint8_t> a(out_cap), b(out_cap), want(bytes);
            CHECK(hipMemcpy(a.data(), d_out[0], out_cap, hipMemcpyDeviceToHost));
            CHECK(hipMemcpy(b.data(), d_out[1], out_cap, hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < n; ++i) {
                const ls::CloudSources src = ls::cloud_sources(&points[(size_t)i * 8], &hits[(size_t)i * 4], false, 0u, col[i % H], chan[i / H], V, H);
                ls::cloud_format_record(fmt, src, want.data() + (size_t)i * step);
            }
            bool same = std::memcmp(a.data(), want.data(), bytes) == 0 && std::memcmp(b.data(), want.data(), bytes) == 0;
            for (size_t k = bytes; k < out_cap; ++k) same = same && a[k] == 0xAB && b[k] == 0xAB;
            if (!same) {
                std::fprintf(stderr, "step %u organized %d: the forms and the host disagree\n", step, organized);
                return 1;
            }
            std::vector<float> ms[3];
            for (int v = 0; v < 3; ++v)
                for (int k = 0; k < 5; ++k) run(v);   // warm-up
            CHECK(hipStreamSynchronize(s));
            for (int r = 0; r < rounds; ++r)
                for (int v = 0; v < 3; ++v) {
                    CHECK(hipEventRecord(e0, s));
                    for (int k = 0; k < reps; ++k) run(v);
                    CHECK(hipEventRecord(e1, s));
                    CHECK(hipEventSynchronize(e1));
                    float t = 0.0f;
                    CHECK(hipEventElapsedTime(&t, e0, e1));
                    ms[v].push_back(t / (float)reps);
                }
            CHECK(hipGetLastError());
            std::printf("%s  {\"step\": %u, \"organized\": %d", first ? "" : ",\n", step, organized);
            first = false;
            const char *names[3] = {"naive", "staged", "copy"};
            for (int v = 0; v < 3; ++v) {
                std::sort(ms[v].begin(), ms[v].end());
                std::printf(", \"%s_us\": {\"median\": %.2f, \"min\": %.2f, \"max\": %.2f}", names[v], 1e3f * ms[v][ms[v].size() / 2], 1e3f * ms[v].front(),
                            1e3f * ms[v].back());
            }
            std::printf("}");
        }
    std::printf("\n]}\n");
    return 0;
}
