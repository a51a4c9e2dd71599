// motion_example.cpp -- the reference's whole per-frame sequence (main.cpp:1786-1825) from files, without
// libmmd: model + rig from a .pmx / .pmd, motion from a .vmd, every step on the GPU behind the C ABI.
//   g++ -std=c++17 -O2 motion_example.cpp -I../../include -L.. -lmmdx -Wl,-rpath,'$ORIGIN/..' -o motion_example
//   ./motion_example model.pmx motion.vmd [frames [hz]]
// With `hz` the loop runs at that display rate: step n seeks to n / hz seconds (MotionPlayer::SeekTime) instead of frame n.
//   ./motion_example --crowd instances hz model.pmx clip0.vmd [clip1.vmd ...]
// Crowd mode (mmdx::MotionSet): the motions are the clips of one bank, instance i plays clip i % clips at i / hz seconds; one
// call each gives every instance's palette and morph rates; then mmdx::Animator runs the crowd's clocks on the device for 60 steps,
// walks it (root motion) and, at the end, walks and turns it (root motion with rotation deltas).
// Prints per-run checksums so tests can compare with the Python path over the same C ABI.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mmdx_poser.hpp"

static uint64_t checksum(const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

static int crowd(int argc, char **argv) {
    if (argc < 6) { std::printf("usage: %s --crowd instances hz model.pmx|.pmd clip0.vmd [clip1.vmd ...]\n", argv[0]); return 64; }
    const uint32_t ni = uint32_t(std::atoi(argv[2]));
    const double hz = std::atof(argv[3]);
    std::unique_ptr<mmdx::Poser> poser(mmdx::Poser::FromFile(argv[4]));
    std::vector<std::unique_ptr<mmdx::Motion>> motions;
    std::vector<const mmdx::Motion *> clips_of;
    for (int a = 5; a < argc; ++a) {
        motions.emplace_back(new mmdx::Motion(argv[a]));
        clips_of.push_back(motions.back().get());
    }
    mmdx::MotionSet set(clips_of, *poser);
    // the same motions in place: bone 0 keeps no translation (the walking crowd at the end plays these)
    const uint32_t all_axes = MMDX_ROOT_X | MMDX_ROOT_Y | MMDX_ROOT_Z;
    mmdx::MotionSet in_place(clips_of, *poser, 0, all_axes);
    // ... and with bone 0's rotation taken out as well (the turning crowd at the very end plays these)
    mmdx::MotionSet in_place_turn(clips_of, *poser, 0, all_axes, true);
    motions.clear();                          // the sets copied what they need
    const uint32_t nc = set.clip_count();
    std::vector<uint32_t> clips(ni);
    std::vector<double> times(ni);
    for (uint32_t i = 0; i < ni; ++i) { clips[i] = i % nc; times[i] = double(i) / hz; }
    std::vector<float> palettes(size_t(ni) * poser->bone_count() * 16), rates(size_t(ni) * poser->morph_count());
    set.SeekTimePalettes(ni, clips.data(), times.data(), palettes.data());
    set.SeekTimeMorphRates(ni, clips.data(), times.data(), rates.data());
    const uint64_t h = checksum(palettes.data(), palettes.size() * 4) * 31 + checksum(rates.data(), rates.size() * 4);
    std::printf("crowd=%u clips=%u nb=%u nm=%u checksum=%016llx\n", ni, nc, poser->bone_count(), poser->morph_count(),
                (unsigned long long)h);
    // where every instance stands: 12 units apart along x, unrotated -- one pose {tx, ty, tz, 0, qx, qy, qz, qw} per instance
    std::vector<float> where(size_t(ni) * 8, 0.f), placed(palettes.size());
    for (uint32_t i = 0; i < ni; ++i) { where[8 * i] = 12.f * float(i); where[8 * i + 7] = 1.f; }
    set.PlacePalettes(ni, palettes.data(), where.data(), placed.data());
    std::fprintf(stderr, "placed checksum=%016llx\n", (unsigned long long)checksum(placed.data(), placed.size() * 4));
    // the same crowd on its own clocks (mmdx::Animator): every instance starts its clip at once, every other one asks for a
    // half-second fade to the next clip after 30 steps; 60 steps of 1 / hz, one launch each, the palettes from the animator's arrays
    mmdx::Animator animator(set, ni);
    std::vector<uint32_t> ids(ni), next;
    for (uint32_t i = 0; i < ni; ++i) ids[i] = i;
    animator.Request(ni, ids.data(), clips.data());
    void *d_palettes = nullptr;
    mmdx::check(mmdx_device_malloc(&d_palettes, palettes.size() * 4));
    ids.clear();
    for (uint32_t i = 0; i < ni; i += 2) { ids.push_back(i); next.push_back((i + 1) % nc); }
    const std::vector<float> fades(ids.size(), 0.5f);
    for (int step = 0; step < 60; ++step) {
        if (step == 30) animator.Request(uint32_t(ids.size()), ids.data(), next.data(), fades.data());
        animator.Advance(1.0 / hz);
        set.BlendTimePalettes(animator.operands(), static_cast<float *>(d_palettes));
    }
    mmdx::check(mmdx_sync(poser->handle()));          // the steps ran on the poser's stream; the copy below does not wait for it
    mmdx::check(mmdx_memcpy_d2h(palettes.data(), d_palettes, palettes.size() * 4));
    mmdx::check(mmdx_device_free(d_palettes));
    std::vector<double> clock(ni);
    std::vector<uint32_t> loops(ni);
    mmdx_animator_arrays state{};
    state.times_a = clock.data(); state.loops = loops.data();
    animator.GetState(state);
    std::fprintf(stderr, "animated checksum=%016llx clock[0]=%.6f loops[0]=%u\n", (unsigned long long)checksum(palettes.data(), palettes.size() * 4),
                 clock[0], loops[0]);
    // the crowd walks (root motion): the poses come from the motions in place, and the placements -- in device memory, turned a
    // little more from one instance to the next -- take what `set` moves bone 0 by in every step.  Step = RootMotion, then Advance.
    mmdx::Animator walker(in_place, ni);
    for (uint32_t i = 0; i < ni; ++i) {
        const float half = 0.05f * float(i);
        where[8 * i + 5] = half; where[8 * i + 7] = 1.f - half * half;       // a heading about y, not normalised
    }
    ids.resize(ni);
    for (uint32_t i = 0; i < ni; ++i) ids[i] = i;
    walker.Request(ni, ids.data(), clips.data());
    void *d_where = nullptr, *d_walk = nullptr;
    mmdx::check(mmdx_device_malloc(&d_where, where.size() * 4));
    mmdx::check(mmdx_device_malloc(&d_walk, palettes.size() * 4));
    mmdx::check(mmdx_memcpy_h2d(d_where, where.data(), where.size() * 4));
    for (int step = 0; step < 60; ++step) {
        walker.Step(set, 0, all_axes, static_cast<float *>(d_where), 1.0 / hz);
        in_place.BlendTimePalettes(walker.operands(), static_cast<float *>(d_walk));
        in_place.PlacePalettes(ni, static_cast<float *>(d_walk), static_cast<float *>(d_where), static_cast<float *>(d_walk), false, true);
    }
    mmdx::check(mmdx_sync(poser->handle()));
    mmdx::check(mmdx_memcpy_d2h(palettes.data(), d_walk, palettes.size() * 4));
    mmdx::check(mmdx_memcpy_d2h(where.data(), d_where, where.size() * 4));
    mmdx::check(mmdx_device_free(d_walk));
    mmdx::check(mmdx_device_free(d_where));
    std::fprintf(stderr, "walked checksum=%016llx where=%016llx\n", (unsigned long long)checksum(palettes.data(), palettes.size() * 4),
                 (unsigned long long)checksum(where.data(), where.size() * 4));
    // an additive layer: every instance keeps playing its clip and gets, one and a half times over, what the NEXT clip does half a
    // second in relative to that clip's own first frame.  The reference rows are the clips at time 0.
    const uint32_t nb = poser->bone_count(), nm = poser->morph_count();
    std::vector<uint32_t> every(nc), layer(ni);
    const std::vector<double> zero(nc, 0.0), half_second(ni, 0.5);
    for (uint32_t c = 0; c < nc; ++c) every[c] = c;
    for (uint32_t i = 0; i < ni; ++i) layer[i] = (clips[i] + 1) % nc;
    std::vector<float> base(size_t(ni) * nb * 8), over(base.size()), refs(size_t(nc) * nb * 8), rate_over(rates.size()), rate_refs(size_t(nc) * nm);
    set.SeekTimePoses(ni, clips.data(), times.data(), base.data());
    set.SeekTimePoses(ni, layer.data(), half_second.data(), over.data());
    set.SeekTimePoses(nc, every.data(), zero.data(), refs.data());
    set.SeekTimeMorphRates(ni, layer.data(), half_second.data(), rate_over.data());
    set.SeekTimeMorphRates(nc, every.data(), zero.data(), rate_refs.data());
    const std::vector<float> more(ni, 1.5f);
    set.AddPoses(ni, nb, base.data(), over.data(), more.data(), nullptr, nullptr, 0, layer.data(), refs.data(), nc, base.data());
    set.AddRates(ni, nm, rates.data(), rate_over.data(), more.data(), nullptr, nullptr, 0, layer.data(), rate_refs.data(), nc, rates.data());
    std::fprintf(stderr, "layered checksum=%016llx rates=%016llx\n", (unsigned long long)checksum(base.data(), base.size() * 4),
                 (unsigned long long)checksum(rates.data(), rates.size() * 4));
    // the crowd walks and turns (root motion with rotation deltas): the poses come from the motions with bone 0's translation AND
    // rotation taken out, and each placement follows bone 0 of `set` as a rigid frame -- its heading is multiplied by the bone's
    // rotation delta and normalised.  StepTurn = RootTurn, then Advance.
    mmdx::Animator turner(in_place_turn, ni);
    std::fill(where.begin(), where.end(), 0.f);
    for (uint32_t i = 0; i < ni; ++i) {
        const float half = 0.05f * float(i);
        where[8 * i] = 12.f * float(i); where[8 * i + 5] = half; where[8 * i + 7] = 1.f - half * half;
    }
    turner.Request(ni, ids.data(), clips.data());
    void *d_turn = nullptr;
    mmdx::check(mmdx_device_malloc(&d_where, where.size() * 4));
    mmdx::check(mmdx_device_malloc(&d_turn, palettes.size() * 4));
    mmdx::check(mmdx_memcpy_h2d(d_where, where.data(), where.size() * 4));
    for (int step = 0; step < 60; ++step) {
        turner.StepTurn(set, 0, all_axes, static_cast<float *>(d_where), 1.0 / hz, true);
        in_place_turn.BlendTimePalettes(turner.operands(), static_cast<float *>(d_turn));
        in_place_turn.PlacePalettes(ni, static_cast<float *>(d_turn), static_cast<float *>(d_where), static_cast<float *>(d_turn), false, true);
    }
    mmdx::check(mmdx_sync(poser->handle()));
    mmdx::check(mmdx_memcpy_d2h(palettes.data(), d_turn, palettes.size() * 4));
    mmdx::check(mmdx_memcpy_d2h(where.data(), d_where, where.size() * 4));
    mmdx::check(mmdx_device_free(d_turn));
    mmdx::check(mmdx_device_free(d_where));
    std::fprintf(stderr, "turned checksum=%016llx where=%016llx\n", (unsigned long long)checksum(palettes.data(), palettes.size() * 4),
                 (unsigned long long)checksum(where.data(), where.size() * 4));
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--crowd")) {
        try {
            return crowd(argc, argv);
        } catch (const mmdx::Error &e) {
            std::printf("mmdx error %d: %s\n", int(e.status), e.what());
            return 1;
        }
    }
    if (argc < 3) { std::printf("usage: %s model.pmx|.pmd motion.vmd [frames [hz]]\n", argv[0]); return 64; }
    try {
        std::unique_ptr<mmdx::Poser> poser(mmdx::Poser::FromFile(argv[1]));
        mmdx::Motion motion(argv[2]);
        mmdx::MotionPlayer player(motion, *poser);
        const size_t frames = argc > 3 ? size_t(std::atoi(argv[3])) : motion.GetLength() + 1;
        const double hz = argc > 4 ? std::atof(argv[4]) : 0.0;
        std::vector<mmdx::Vertex> vertices;
        uint64_t h = 0;
        for (size_t frame = 0; frame < frames; ++frame) {
            poser->ResetPosing();                 // main.cpp:1788
            if (hz > 0.0) player.SeekTime(double(frame) / hz);   // a display-rate loop: the time, not a frame number
            else player.SeekFrame(frame);         // :1795
            poser->PrePhysicsPosing();            // :1801  (physics would React() here and overwrite its bones)
            poser->PostPhysicsPosing();           // :1810
            poser->Deform();                      // :1821
            poser->UpdateDeformedVertices(vertices);   // :1824
            h = h * 31 + checksum(vertices.data(), vertices.size() * sizeof(mmdx::Vertex)) +
                checksum(poser->pose_image.normals.data(), size_t(poser->vertex_count()) * 12);
        }
        std::printf("frames=%zu nv=%u nb=%u mapped_bones=%u checksum=%016llx\n", frames, poser->vertex_count(),
                    poser->bone_count(), player.mapped_bones(), (unsigned long long)h);
    } catch (const mmdx::Error &e) {
        std::printf("mmdx error %d: %s\n", int(e.status), e.what());
        return 1;
    }
    return 0;
}
