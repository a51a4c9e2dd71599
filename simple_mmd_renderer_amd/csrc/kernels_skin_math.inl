// kernels_skin_math.inl -- the skinning arithmetic of the deform kernels: binary16 conversion, the palette matrix on packed f32
// pairs (M12) with the reference's blends and transforms, the vertex's static data (Slot) and its blended matrix (skin_matrix).
// A piece of kernels.hip (included inside namespace mmdx { namespace {), compiled with it, plain and fast-math.

constexpr float kLerpLo = 1e-7f;                  // float(mmd_math_const_eps)
constexpr float kLerpHi = 0.99999988f;            // float(1.0 - mmd_math_const_eps)

__device__ __forceinline__ float h2f(uint32_t bits16) {
    return float(__builtin_bit_cast(_Float16, (unsigned short)bits16));
}
__device__ __forceinline__ unsigned short f2h(float x) {
    return __builtin_bit_cast(unsigned short, _Float16(x));  // v_cvt_f16_f32, round to nearest even
}

// ---- matrix blend + mat*vec, reference operation order, on PACKED f32 pairs ------------------------
// A wave64 issues one VALU instruction per 4 cycles, so at the occupancy this kernel runs at the
// number of VALU instructions is what counts: v_pk_mul_f32 / v_pk_add_f32 do two IEEE f32 operations
// per instruction (each half rounded exactly like v_mul_f32 / v_add_f32).  The palette is laid out
// in LDS so that every operand pair is an aligned register pair -- no shuffles:
//     entry = 3 x float4 = {m00 m01 | m10 m11} {m20 m21 | m30 m31} {m02 m12 | m22 m32}
// (M[r][c], row-vector convention; column 3 of the matrix is never read by the path).
typedef float v2f __attribute__((ext_vector_type(2)));

struct M12 {
    v2f p0, p1, p2, p3;  // (m_r0, m_r1) for r = 0..3
    v2f q0, q1;          // (m02, m12), (m22, m32)
};

__device__ __forceinline__ M12 load_m12(const float4 *P, uint32_t b) {
    const float4 A = P[b], B = P[b + 1], C = P[b + 2];
    M12 m;
    m.p0 = v2f{A.x, A.y}; m.p1 = v2f{A.z, A.w};
    m.p2 = v2f{B.x, B.y}; m.p3 = v2f{B.z, B.w};
    m.q0 = v2f{C.x, C.y}; m.q1 = v2f{C.z, C.w};
    return m;
}
// Lerp(a, b)[l] interior: (1-l)*a + l*b per element (math_impl.inl:1253; s*M :1004-1023, M+M :944-963)
__device__ __forceinline__ M12 blend2(const M12 &a, const M12 &b, float s1, float l) {
    M12 r;
    r.p0 = a.p0 * s1 + b.p0 * l; r.p1 = a.p1 * s1 + b.p1 * l;
    r.p2 = a.p2 * s1 + b.p2 * l; r.p3 = a.p3 * s1 + b.p3 * l;
    r.q0 = a.q0 * s1 + b.q0 * l; r.q1 = a.q1 * s1 + b.q1 * l;
    return r;
}
// BDEF4: ((m0*w0 + m1*w1) + m2*w2) + m3*w3 per element (poser_impl.inl:433; weights not normalised), evaluated in steps:
// a*wa + b*wb, then t + c*wc
__device__ __forceinline__ M12 mul_add(const M12 &a, float wa, const M12 &b, float wb) {
    M12 r;
    r.p0 = a.p0 * wa + b.p0 * wb; r.p1 = a.p1 * wa + b.p1 * wb;
    r.p2 = a.p2 * wa + b.p2 * wb; r.p3 = a.p3 * wa + b.p3 * wb;
    r.q0 = a.q0 * wa + b.q0 * wb; r.q1 = a.q1 * wa + b.q1 * wb;
    return r;
}
__device__ __forceinline__ M12 add_mul(const M12 &t, const M12 &c, float wc) {
    M12 r;
    r.p0 = t.p0 + c.p0 * wc; r.p1 = t.p1 + c.p1 * wc;
    r.p2 = t.p2 + c.p2 * wc; r.p3 = t.p3 + c.p3 * wc;
    r.q0 = t.q0 + c.q0 * wc; r.q1 = t.q1 + c.q1 * wc;
    return r;
}
// transform(): out[j] = ((x*m0j + y*m1j) + z*m2j) + m3j   (math_impl.inl:1039-1045)
__device__ __forceinline__ void xform_pos(const M12 &m, v2f xy, float z, v2f &oxy, float &oz) {
    oxy = ((m.p0 * xy.x + m.p1 * xy.y) + m.p2 * z) + m.p3;
    const v2f t = m.q0 * xy;
    oz = ((t.x + t.y) + z * m.q1.x) + m.q1.y;
}
// rotate(): out[j] = (x*m0j + y*m1j) + z*m2j   (math_impl.inl:1032-1038) -- same matrix, no
// inverse transpose, no renormalisation
__device__ __forceinline__ void xform_nrm(const M12 &m, v2f xy, float z, v2f &oxy, float &oz) {
    oxy = (m.p0 * xy.x + m.p1 * xy.y) + m.p2 * z;
    const v2f t = m.q0 * xy;
    oz = (t.x + t.y) + z * m.q1.x;
}

// The static data of one vertex (sorted slot) in registers: what load_slot (kernels_setup.inl) fills and skin_matrix reads.
struct Slot {
    v2f pxy, nxy, uv;
    float pz, nz;
    float w0, w1, w2, w3;
    uint32_t b0, b1, b2, b3;  // float4 index of the bone's entry inside one instance's palette
    uint32_t perm;
    uint32_t rb, rlen;        // morph-table row: first entry (incl. lane), padded length
    int cls;
    bool act;
};

// The vertex's blended palette matrix: BDEF1 the bone's, BDEF2-like Lerp(S[b1], S[b0])[w] with the epsilon short circuits,
// BDEF4 ((S0*w0 + S1*w1) + S2*w2) + S3*w3 (poser_impl.inl:412-434).  P = the instance's palette in LDS.
__device__ __forceinline__ M12 skin_matrix(const Slot &q, const float4 *P) {
    M12 m;
    if (q.cls == 0) {
        m = load_m12(P, q.b0);
    } else if (q.cls == 1) {
        // Lerp(S[b1], S[b0])[w]  (poser_impl.inl:420-422, math_impl.inl:1246-1254)
        const M12 a = load_m12(P, q.b1), e = load_m12(P, q.b0);
        const float l = q.w0;
        m = blend2(a, e, 1.0f - l, l);
        // epsilon short-circuits: rare, so only waves that hold such a weight pay for them
        const bool lo = l < kLerpLo, hi = l > kLerpHi;
        if (__builtin_amdgcn_ballot_w64(lo || hi) != 0) {
            if (lo) m = a;
            else if (hi) m = e;
        }
    } else {
        // ((S0*w0 + S1*w1) + S2*w2) + S3*w3, two palette entries in registers at a time: the scheduler would
        // otherwise issue all twelve LDS reads first and hold four matrices (48 VGPRs) at once -- the peak
        // of the kernel's register pressure
        {
            const M12 a = load_m12(P, q.b0), b = load_m12(P, q.b1);
            m = mul_add(a, q.w0, b, q.w1);
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            const M12 c = load_m12(P, q.b2);
            m = add_mul(m, c, q.w2);
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            const M12 d = load_m12(P, q.b3);
            m = add_mul(m, d, q.w3);
        }
    }
    return m;
}
