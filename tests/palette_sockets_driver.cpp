// tests/palette_sockets_driver.cpp -- TEST INFRASTRUCTURE ONLY: mmdx_palette_sockets (include/mmdx.h) computed by the real libmmd.
// A stand-alone program: every line of stdin is one row -- the form of the socket's offset (0 = none, 1 = pose, 2 = matrix), the 16
// floats of a skinning matrix S, 4 floats of the bone's rest position p (the fourth is not used) and 16 floats of an offset (a pose
// uses the first 8: tx ty tz _ qx qy qz qw), each float as the 8 hex digits of its bit pattern -- and every line of stdout the 16
// floats of the socket's matrix in the same notation.
//   G            MakeIdentity(), then G.r.v[3].downgrade.vector3d = p: how libmmd builds a bone's global_offset_matrix_inv_
//                (L/motion/poser_impl.inl:36-37, :497);
//   pose form    O = Quaternionf::ToRotateMatrix() (L/util/math_impl.inl:540-563), then O.r.v[3].downgrade.vector3d = translation
//                (L/motion/poser_impl.inl:161-162);
//   matrix form  O.v[0..15] = the 16 floats;
//   the result   G * S, or O * (G * S): Matrix4f::operator* (L/util/math_impl.inl:984-1003).
// libmmd is #included by path at build time (tests/palette_sockets_ref.py compiles this file with g++ -O2 -ffp-contract=off);
// nothing built from it is committed.  (L/ = 3rd_party/libmmd/include/mmd/)

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
        float in[36];
        for (int k = 0; k < 36; ++k) {
            unsigned u;
            if (std::scanf("%x", &u) != 1) return 2;
            in[k] = from_bits(u);
        }
        mmd::Matrix4f s, g, o;
        for (int k = 0; k < 16; ++k) s.v[k] = in[k];
        mmd::Vector3f p;
        for (int k = 0; k < 3; ++k) p.v[k] = in[16 + k];
        g.MakeIdentity();
        g.r.v[3].downgrade.vector3d = p;
        mmd::Matrix4f r = g * s;
        const float *off = in + 20;
        if (form == 1) {
            mmd::Vector4f q;
            for (int k = 0; k < 4; ++k) q.v[k] = off[4 + k];
            mmd::Vector3f t;
            for (int k = 0; k < 3; ++k) t.v[k] = off[k];
            o = q.q.ToRotateMatrix();
            o.r.v[3].downgrade.vector3d = t;
            r = o * r;
        } else if (form == 2) {
            for (int k = 0; k < 16; ++k) o.v[k] = off[k];
            r = o * r;
        }
        for (int k = 0; k < 16; ++k) std::printf("%08x%c", to_bits(r.v[k]), k == 15 ? '\n' : ' ');
    }
    return 0;
}
