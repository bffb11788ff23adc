// The GPU context of libeigkl_hip.so: its lifetime, streams and the pinned
// upload staging (host code over the HIP runtime).
#include "ctx.hpp"

using namespace ek::rt;

Uploader::Uploader(ek_ctx* ctx, hipStream_t st, size_t total)
    : c(ctx), s(st), buf(st == ctx->kstream ? ctx->kup : ctx->up), cap(st == ctx->kstream ? ctx->kup_bytes : ctx->up_bytes) {
    // alignment slack: every put starts on a 64-byte line, so up to eight of
    // them fit whatever their sizes (a two-node partition's four puts hold 18
    // bytes and end at offset 200)
    total = total * 2 + 64 * 8;
    if (cap < total) {
        // the arena's previous user drained its stream before returning
        if (buf) HIPCHK(hipHostFree(buf));
        buf = nullptr;
        cap = 0;
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&buf), total, hipHostMallocDefault));
        cap = total;
    }
}

void ek::ctx_ranks(ek_ctx* c, int* rank, int* nranks) {
    if (!c) fail(EK_EINVAL, "null ek_ctx");
    if (rank) *rank = c->rank;
    if (nranks) *nranks = c->nranks;
}

extern "C" {

int ek_device_count(int* count) {
    EK_TRY
    int c = 0;
    const hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) c = 0;
    if (count) *count = c;
    return EK_OK;
    EK_CATCH
}

int ek_init(int device, ek_ctx** out) {
    EK_TRY
    if (!out) ek::fail(EK_EINVAL, "ek_init: null out");
    int cnt = 0;
    ek::cold_stamp("hip_first_call");
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) ek::fail(EK_EHIP, "no HIP device available (no CPU fallback)");
    ek::cold_stamp("hip_device_count");
    if (device < 0 || device >= cnt) ek::fail(EK_EINVAL, "device %d out of range [0,%d)", device, cnt);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    ek::cold_stamp("hip_props");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        ek::fail(EK_EHIP, "device %d is %s; this build targets gfx950 (MI355X)", device, prop.gcnArchName);
    auto c = std::make_unique<ek_ctx>();
    c->device = device;
    c->num_cu = std::max(1, prop.multiProcessorCount);
    HIPCHK(hipSetDevice(device));
    ek::cold_stamp("hip_set_device");
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    ek::cold_stamp("hip_stream0");
    HIPCHK(hipStreamCreateWithFlags(&c->kstream, hipStreamNonBlocking));
    ek::cold_stamp("hip_streams");
    *out = c.release();
    return EK_OK;
    EK_CATCH
}

void ek_destroy(ek_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    // drain every stream before anything it may still copy from is freed
    // (an error exit can leave async copies of the pinned buffers queued)
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->kstream);
    if (c->cstream) (void)hipStreamSynchronize(c->cstream);
    if (c->comm) ncclCommDestroy(c->comm);
    for (auto e : c->spmv_ev) (void)hipEventDestroy(e);
    for (auto e : c->cm_ev) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) {
        if (i == 0 && c->fin_ev) (void)hipEventDestroy(c->fin_ev);
        if (c->chk_done[i]) (void)hipEventDestroy(c->chk_done[i]);
        if (c->chk_copied[i]) (void)hipEventDestroy(c->chk_copied[i]);
    }
    if (c->cstream) (void)hipStreamDestroy(c->cstream);
    if (c->gstream) {
        (void)hipStreamSynchronize(c->gstream);
        (void)hipStreamDestroy(c->gstream);
    }
    for (auto e : c->ag_ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& g : c->lz_graphs) (void)hipGraphExecDestroy(g.second);
    (void)hipStreamDestroy(c->kstream);
    (void)hipStreamDestroy(c->stream);
    if (c->chk_pin) (void)hipHostFree(c->chk_pin);
    if (c->chk_word) (void)hipHostFree(c->chk_word);
    if (c->q_pin) (void)hipHostFree(c->q_pin);
    if (c->pin) (void)hipHostFree(c->pin);
    if (c->stage) (void)hipHostFree(c->stage);
    if (c->up) (void)hipHostFree(c->up);
    if (c->kup) (void)hipHostFree(c->kup);
    delete c;
}

int ek_get_stream(ek_ctx* c, void** s) {
    EK_TRY
    check_ctx(c);
    if (s) *s = c->stream;
    return EK_OK;
    EK_CATCH
}

int ek_synchronize(ek_ctx* c) {
    EK_TRY
    check_ctx(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    return EK_OK;
    EK_CATCH
}

}  // extern "C"
