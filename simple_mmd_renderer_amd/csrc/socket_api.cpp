// socket_api.cpp -- the socket set handle and mmdx_palette_sockets (include/mmdx.h): the table of socket_table.hpp uploaded at
// creation, argument validation on the host, host operands through the model's scratch the way mmdx_palette_place takes them (its
// place_in / place_out: both calls run on the model's stream and wait before they return), the instance list of the select form, and
// the launch (socket_kernels.hip) on the model's stream.
#include <memory>
#include <mutex>
#include <string>

#include "api_internal.hpp"
#include "socket_kernels.hpp"

using namespace mmdx;

struct mmdx_socket_set_s {
    mmdx_model_t model = nullptr;                 // nullptr once the model has been destroyed (guarded by g_sets_mu)
    uint32_t ns = 0, nb = 0, n_offsets = 0;
    int device = -1;                              // the model's; -1 = host-only
    std::vector<SocketEntry> host;                // the table as uploaded
    DevBuf table;                                 // static: [ns] SocketEntry
    DevBuf sel;                                   // a host list: {live count, ids[live]}
    std::vector<uint32_t> sel_host;               // ... its source, alive until the copy has left it
    GraphPin pin;                                 // recorded graphs that hold these addresses
    mmdx_socket_set_s() { table.pin = sel.pin = &pin; }
};

namespace {

std::mutex g_sets_mu;                             // set <-> model links (rare operations: create, destroy)
std::vector<mmdx_socket_set_s *> g_sets;

bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace

// api.cpp, when a model goes: its sets stay valid handles that refuse every call
void mmdx::socket_sets_forget_model(mmdx_model_s *m) {
    std::lock_guard<std::mutex> lk(g_sets_mu);
    for (mmdx_socket_set_s *s : g_sets)
        if (s->model == m) s->model = nullptr;
}

extern "C" {

mmdx_status mmdx_socket_set_create(mmdx_model_t model, const mmdx_socket_set_desc *desc, mmdx_socket_set_t *out_set) {
    if (!out_set) return fail(MMDX_ERR_INVALID_ARGUMENT, "out_set is NULL");
    *out_set = nullptr;
    if (!model || !desc) return fail(MMDX_ERR_INVALID_ARGUMENT, "model / desc is NULL");
    try {
        std::unique_ptr<mmdx_socket_set_s> s(new mmdx_socket_set_s);
        if (mmdx_status r = socket_table_build(desc, model->plan.nb, &s->host, &s->n_offsets)) return r;
        s->model = model;
        s->ns = desc->n_sockets;
        s->nb = model->plan.nb;
        s->device = model->device;
        if (s->device >= 0) {
            HIP_TRY(hipSetDevice(s->device));
            if (hipError_t e = s->table.upload(s->host)) {
                s->table.release();
                return hip_fail(e, "socket table upload");
            }
        }
        std::lock_guard<std::mutex> lk(g_sets_mu);
        g_sets.push_back(s.get());
        *out_set = s.release();
    } catch (const std::bad_alloc &) {
        return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    return MMDX_OK;
}

void mmdx_socket_set_destroy(mmdx_socket_set_t set) {
    if (!set) return;
    {
        std::lock_guard<std::mutex> lk(g_sets_mu);
        g_sets.erase(std::remove(g_sets.begin(), g_sets.end(), set), g_sets.end());
    }
    graph_drop_handle(&set->pin);
    if (set->device >= 0) (void)hipSetDevice(set->device);
    set->table.release();
    set->sel.release();
    delete set;
}

mmdx_status mmdx_socket_set_get_info(mmdx_socket_set_t set, mmdx_socket_set_info *info) {
    if (!set || !info || info->struct_size != sizeof(mmdx_socket_set_info))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or mmdx_socket_set_info.struct_size mismatch");
    info->n_sockets = set->ns;
    info->n_offsets = set->n_offsets;
    info->n_bones = set->nb;
    info->device_ordinal = set->device;
    info->reserved0 = 0;
    return MMDX_OK;
}

mmdx_status mmdx_palette_sockets(mmdx_socket_set_t set, const mmdx_sockets_args *a) {
    if (!set || !a) return fail(MMDX_ERR_INVALID_ARGUMENT, "set / args is NULL");
    if (a->struct_size != sizeof(mmdx_sockets_args)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_sockets_args.struct_size mismatch");
    const uint32_t on_device = MMDX_PALETTE_ON_DEVICE | MMDX_OUT_ON_DEVICE;
    if (a->flags & ~on_device) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits in mmdx_sockets_args.flags");
    if (a->reserved0 != 0) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_sockets_args.reserved0 must be 0");
    const mmdx_instance_select *sel = a->select;
    if (sel)
        if (mmdx_status r = list_header_check(sel)) return r;
    mmdx_model_t m;
    {
        std::lock_guard<std::mutex> lk(g_sets_mu);
        m = set->model;
    }
    if (!m) return fail(MMDX_ERR_INVALID_ARGUMENT, "the model this socket set was created on has been destroyed");
    const uint32_t ni = a->n_instances, nb = set->nb, ns = set->ns;
    if (!ni) return MMDX_OK;
    if (!a->palettes || !a->out_sockets) return fail(MMDX_ERR_INVALID_ARGUMENT, "palettes / out_sockets is NULL");
    const size_t pal_bytes = size_t(ni) * nb * 16 * sizeof(float), out_bytes = size_t(ns) * ni * 16 * sizeof(float);
    if (overlap(a->palettes, pal_bytes, a->out_sockets, out_bytes)) return fail(MMDX_ERR_INVALID_ARGUMENT, "out_sockets overlaps palettes");
    uintptr_t align16 = 0;
    if (a->flags & MMDX_PALETTE_ON_DEVICE) align16 |= reinterpret_cast<uintptr_t>(a->palettes);
    if (a->flags & MMDX_OUT_ON_DEVICE) align16 |= reinterpret_cast<uintptr_t>(a->out_sockets);
    if (align16 & 15) return fail(MMDX_ERR_INVALID_ARGUMENT, "device palettes / out_sockets must be 16-byte aligned");
    if (ni > kSocketMaxCells || (sel && sel->n_ids > kSocketMaxCells))
        return fail(MMDX_ERR_UNSUPPORTED, "mmdx_palette_sockets: more than 2^23 instances or list positions in one call");
    uint32_t live_host = 0;
    if (sel) {
        if (mmdx_status r = list_placement_check(sel, m->capturing)) return r;
        if ((a->flags & on_device) != on_device)
            return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_palette_sockets with a select list takes palettes and out_sockets in device memory "
                                                   "only (the staging copies of host operands move whole arrays)");
        if (mmdx_status r = host_list_check(sel, ni, live_host)) return r;
    }
    if (mmdx_status r = model_call_begin(m, a->flags, on_device, "while a graph is being recorded palettes and out_sockets must both "
                                                                 "be in device memory"))
        return r;
    hipStream_t st = m->stream;
    graph_note_handle(m, &set->pin);
    SocketLaunch p{a->palettes, static_cast<const SocketEntry *>(set->table.ptr), a->out_sockets, ni, nb, ns, set->n_offsets != 0};
    InstanceList list{nullptr, nullptr, ni};
    uint32_t cells = ni;
    if (sel) {
        list = InstanceList{sel->ids, sel->count, ni};
        cells = sel->n_ids;
        if (!(sel->flags & MMDX_SELECT_ON_DEVICE)) {
            cells = live_host;
            if (live_host)
                if (mmdx_status r = stage_list(set->sel, set->sel_host, sel->ids, live_host, live_host, st, &list.count, &list.ids)) return r;
        }
        if (!cells) return MMDX_OK;
    }
    if (!(a->flags & MMDX_PALETTE_ON_DEVICE)) {
        if (mmdx_status r = stage_in(m->place_in, a->palettes, pal_bytes, st)) return r;
        p.palettes = static_cast<const float *>(m->place_in.ptr);
    }
    OutRoute o;
    if (mmdx_status r = route_out(a->flags, a->out_sockets, out_bytes, m->place_out, &o)) return r;
    p.out = o.dev;
    HIP_TRY(launch_palette_sockets(p, sel ? &list : nullptr, cells, st));
    const bool borrowed = (a->flags & on_device) != on_device || (sel && !(sel->flags & MMDX_SELECT_ON_DEVICE));
    return finish(a->flags, borrowed, st, o);
}

}  // extern "C"
