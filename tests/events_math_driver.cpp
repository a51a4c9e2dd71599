// events_math_driver.cpp -- csrc/events_math.hpp and csrc/events_table.hpp built for the host: the lines the gfx950 kernels compile,
// run over a state table by a stand-alone program (tests/animator_events_ref.py builds it through tests/host_program.py, plain and
// under the sanitizers, and compares what it writes with the numpy restatement).
//
//   events_math_driver in.bin out.bin
//
// in.bin   u32 ni, nc, n_markers, n_calls, n_lists, has_levels
//          the clip table: f64 length[nc], u32 mode[nc], u32 next[nc], f32 fade[nc]
//          the markers as given to mmdx_event_set_create: n_markers x {f64 time, u32 clip, u32 channel}
//          u32 clips_a[ni], u32 clips_b[ni], f64 times_a[ni], f64 times_b[ni], f32 weights[ni], f32 speed[ni], f32 fade_rate[ni]
//          f64 dt[n_calls], u32 dominant[n_calls], u32 list_mask[4], u32 levels[ni] when has_levels
// out.bin  the markers as the set stores them, u32 first[nc + 1]
//          per call: u32 fired[ni], u32 counts[4], u32 lists[4][ni] (ascending ids, 0xFFFFFFFF behind a count)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../simple_mmd_renderer_amd/csrc/events_math.hpp"
#include "../simple_mmd_renderer_amd/csrc/events_table.hpp"

using namespace mmdx;

template <class T>
static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "events_math_driver: the input is short\n");
        exit(2);
    }
    return v;
}
template <class T>
static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "events_math_driver: cannot write\n");
        exit(2);
    }
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: events_math_driver in.bin out.bin\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "events_math_driver: cannot open the files\n");
        return 2;
    }
    const std::vector<uint32_t> head = take<uint32_t>(in, 6);
    const uint32_t ni = head[0], nc = head[1], nm = head[2], n_calls = head[3], n_lists = head[4], has_levels = head[5];
    const std::vector<double> length = take<double>(in, nc);
    const std::vector<uint32_t> mode = take<uint32_t>(in, nc), next = take<uint32_t>(in, nc);
    const std::vector<float> fade = take<float>(in, nc);
    const std::vector<EventMarker> given = take<EventMarker>(in, nm);
    const std::vector<uint32_t> clips_a = take<uint32_t>(in, ni), clips_b = take<uint32_t>(in, ni);
    const std::vector<double> times_a = take<double>(in, ni), times_b = take<double>(in, ni);
    const std::vector<float> weights = take<float>(in, ni), speed = take<float>(in, ni), fade_rate = take<float>(in, ni);
    const std::vector<double> dts = take<double>(in, n_calls);
    const std::vector<uint32_t> dominant = take<uint32_t>(in, n_calls), list_mask = take<uint32_t>(in, kEventsMaxLists);
    const std::vector<uint32_t> levels = take<uint32_t>(in, has_levels ? ni : 0);
    if (n_lists > kEventsMaxLists) return 2;

    std::vector<EventMarker> sorted;
    std::vector<uint32_t> first;
    events_table_build(given.data(), nm, nc, &sorted, &first);
    put(out, sorted);
    put(out, first);

    const AnimClips k{length.data(), mode.data(), next.data(), fade.data(), nc};
    const EventTable e{sorted.data(), first.data(), nc};
    for (uint32_t call = 0; call < n_calls; ++call) {
        std::vector<uint32_t> fired(ni), counts(kEventsMaxLists, 0), lists(size_t(kEventsMaxLists) * ni, 0xFFFFFFFFu);
        for (uint32_t i = 0; i < ni; ++i)
            fired[i] = events_fired(k, e, clips_a[i], clips_b[i], times_a[i], times_b[i], weights[i], speed[i], fade_rate[i], dts[call],
                                    dominant[call] != 0);
        for (uint32_t l = 0; l < n_lists; ++l)
            for (uint32_t i = 0; i < ni; ++i)
                if (events_in_list(fired[i], list_mask[l], has_levels != 0, has_levels ? levels[i] : 0u)) lists[size_t(l) * ni + counts[l]++] = i;
        put(out, fired);
        put(out, counts);
        put(out, lists);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
