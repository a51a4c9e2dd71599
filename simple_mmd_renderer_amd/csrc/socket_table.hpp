// socket_table.hpp -- a socket set's device table and its host builder: what mmdx_socket_set_create (socket_api.cpp) validates and
// uploads, and what the kernel (socket_kernels.hip) reads per socket.  No HIP here: tests/socket_table_driver.cpp compiles these lines
// with g++ (and under ASan + UBSan).  socket_math.hpp expands a pose-form offset, so the kernel only ever sees matrices and a
// pose-form offset gives the bits of the matrix it expands to.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mmdx.h"
#include "error.hpp"
#include "socket_math.hpp"

namespace mmdx {

constexpr uint32_t kSocketMaxSockets = 65535;       // grid y = socket

struct alignas(16) SocketEntry {                    // 96 bytes, wave-uniform in the kernel: scalar loads
    uint32_t bone, has_offset, pad0, pad1;
    float p[4];                                     // the bone's rest position; p[3] unused
    float o[16];                                    // the local offset matrix; not read when has_offset == 0
};
static_assert(sizeof(SocketEntry) == 96, "the table row is 6 x 16 bytes");

// The table `d` describes for a model of n_bones bones, validated; *n_offsets = how many sockets have an offset.
inline mmdx_status socket_table_build(const mmdx_socket_set_desc *d, uint32_t n_bones, std::vector<SocketEntry> *out, uint32_t *n_offsets) {
    if (!d) return fail(MMDX_ERR_INVALID_ARGUMENT, "desc is NULL");
    if (d->struct_size != sizeof(mmdx_socket_set_desc)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_socket_set_desc.struct_size mismatch");
    if (d->flags & ~uint32_t(MMDX_SOCKET_OFFSET_MATRIX))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits in mmdx_socket_set_desc.flags");
    if (d->reserved0 != 0) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_socket_set_desc.reserved0 must be 0");
    if (!d->n_sockets) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_socket_set_desc.n_sockets == 0");
    if (d->n_sockets > kSocketMaxSockets) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_socket_set_desc.n_sockets is above 65535");
    if (!d->bone || !d->rest_position) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_socket_set_desc.bone / rest_position is NULL");
    if (d->has_offset && !d->offset) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_socket_set_desc.has_offset is given but offset is NULL");
    const bool matrix = (d->flags & MMDX_SOCKET_OFFSET_MATRIX) != 0;
    const size_t stride = matrix ? 16 : MMDX_POSE_FLOATS;
    out->assign(d->n_sockets, SocketEntry{});
    *n_offsets = 0;
    for (uint32_t s = 0; s < d->n_sockets; ++s) {
        SocketEntry &e = (*out)[s];
        if (d->bone[s] >= n_bones)
            return fail(MMDX_ERR_BAD_INDEX, "mmdx_socket_set_desc.bone[" + std::to_string(s) + "] = " + std::to_string(d->bone[s]) +
                                            ": the model has " + std::to_string(n_bones) + " bones");
        e.bone = d->bone[s];
        for (int k = 0; k < 3; ++k) e.p[k] = d->rest_position[size_t(s) * 3 + k];
        if (!d->offset || (d->has_offset && !d->has_offset[s])) continue;
        e.has_offset = 1;
        ++*n_offsets;
        const float *src = d->offset + size_t(s) * stride;
        if (matrix) std::copy(src, src + 16, e.o);
        else socket_offset_from_pose(src, e.o);
    }
    return MMDX_OK;
}

}  // namespace mmdx
