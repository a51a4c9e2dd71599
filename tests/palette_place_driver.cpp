// tests/palette_place_driver.cpp -- TEST INFRASTRUCTURE ONLY: mmdx_palette_place (include/mmdx.h) computed by the real libmmd.
// A stand-alone program: every line of stdin is one row -- the form (0 = pose, 1 = matrix), the 16 floats of a skinning matrix S
// and 16 floats of a placement (a pose uses the first 8: tx ty tz _ qx qy qz qw), each float as the 8 hex digits of its bit
// pattern -- and every line of stdout the 16 floats of S * W in the same notation.
//   pose form    W = Quaternionf::ToRotateMatrix() (L/util/math_impl.inl:540-563), then W.r.v[3].downgrade.vector3d = translation,
//                the two statements libmmd builds a bone's local_matrix_ with (L/motion/poser_impl.inl:161-162), no local offset;
//   matrix form  W.v[0..15] = the 16 floats;
//   the product  Matrix4f::operator* (L/util/math_impl.inl:984-1003).
// libmmd is #included by path at build time (tests/palette_place_ref.py compiles this file with g++ -O2 -ffp-contract=off); nothing
// built from it is committed.  (L/ = 3rd_party/libmmd/include/mmd/)

// The include order of oracle/ref_harness.cpp and of the viewer: <math.h> / <stdlib.h> before mmd.hxx.
#include <math.h>
#include <stdlib.h>

#include <mmd/mmd.hxx>

#include <cstdint>
#include <cstdio>
#include <cstring>

static float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static uint32_t to_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main() {
    unsigned form;
    while (std::scanf("%u", &form) == 1) {
        float in[32];
        for (int k = 0; k < 32; ++k) {
            unsigned u;
            if (std::scanf("%x", &u) != 1) return 2;
            in[k] = from_bits(u);
        }
        mmd::Matrix4f s, w;
        for (int k = 0; k < 16; ++k) s.v[k] = in[k];
        const float *p = in + 16;
        if (form == 0) {
            mmd::Vector4f q;
            for (int k = 0; k < 4; ++k) q.v[k] = p[4 + k];
            mmd::Vector3f t;
            for (int k = 0; k < 3; ++k) t.v[k] = p[k];
            w = q.q.ToRotateMatrix();
            w.r.v[3].downgrade.vector3d = t;
        } else {
            for (int k = 0; k < 16; ++k) w.v[k] = p[k];
        }
        const mmd::Matrix4f r = s * w;
        for (int k = 0; k < 16; ++k) std::printf("%08x%c", to_bits(r.v[k]), k == 15 ? '\n' : ' ');
    }
    return 0;
}
