// gphip_multi.inc -- multi-device handles: the 1-D block-cyclic Cholesky schedule and its one exchange step,
// driven from INSIDE the library (part of gphip.hip's translation unit; SURVEY.md §8b "devices/ndev", §8e).
//
// Who needs this: the reference's callers are ONE Wolfram kernel process (nestedSampling,
// BayesianStatistics.wl:1099-1136) or sub-kernel processes (parallelNestedSampling, :1349-1357).  Neither
// can run a Python/torch schedule, so everything a sharded evaluation needs sits behind the C ABI:
//
//   gphip_create(.., devices, ndev > 1, ..)    ONE process, ndev devices: a "group" handle = one context
//                                              per device + an in-process communicator (ncclCommInitAll)
//   gphip_create_rank(.., rank, world, id, ..) one process PER device (sub-kernels / torchrun ranks):
//                                              ncclCommInitRank on an id from gphip_comm_unique_id
//
// Three axes (SURVEY.md §8e), all reachable through the ordinary entry points of a group handle:
//   (1) theta / posterior samples: gphip_loglik_batch / gphip_predict_samples deal their units to the
//       local devices, one host thread per device, NO collective;
//   (2) test points: after gphip_fit every device holds the whole factor (see "replication" below) and
//       gphip_predict shards the test points, NO collective;
//   (3) one factorisation (N >= option "shard_min_n", default 16384): outer panel j (`panel` tile columns)
//       belongs to rank j % world; per step k
//           owner(k+1), panel stream:  LA(k) on its panel k+1, factor it, pack it
//           everyone,   comm stream:   broadcast of packed panel k+1      <- the ONE exchange step
//           everyone,   main stream:   REST(k) on the owned panels >= k+2 (+ the corner tile on rank 0)
//       i.e. the single-GPU look-ahead schedule with the panel hand-over replaced by a broadcast; the
//       compute steps are the gphip_dist_* calls (same kernels).  Scalars (log det, quad, info) are summed
//       on the host when all ranks are local, by one 4-double ncclAllReduce otherwise.
//
// Replication of L for prediction ("C3"): every rank RECEIVES every factored panel anyway (it needs it for
// its trailing updates), so a fit simply unpacks each received panel into the rank's own workspace: after
// the last broadcast all ranks hold all of L and z = L^-1 r with no further traffic (an all-gather would
// move the same 8 N^2/2 bytes a second time).  The 128-block inverses are rebuilt locally (trtri128).
//
// Communicators: RCCL (bound with dlopen, rccl_dyn.h) -- broadcast of the packed panel as bytes on the
// rank's comm stream, grouped over the local ranks -- or, when every rank is local and RCCL is absent /
// the same device is listed several times (virtual ranks on a 1-GPU box) / GPHIP_COMM=copy, plain
// device-to-device copies issued from each receiver's comm stream.  (GPHIP_COMM=rccl forces the RCCL calls even for
// virtual ranks: only a tests-only collective library accepts that, tests/test_gpu_multiprocess.py.)

#include <thread>

struct gphip_group {
    int world = 1;                         // ranks of the whole job
    std::vector<int> ranks;                // global rank of local member i
    std::vector<gphip_ctx*> members;       // members[0] is the public handle itself
    bool use_rccl = false;
    bool broken = false;                   // a collective call failed: no further sharded evaluations on this handle
    bool two_hop = false;                  // the CURRENT collective operation broadcasts panels as scatter + all-gather (option "bcast_two_hop")
    int replicate = 0;                     // layout of the CURRENT collective operation (options may change between a fit and
                                           // the prediction that streams its factor: that one always runs with 0)
    unsigned long fit_id = 0;              // number of the last fit on this handle: members carry it while they hold that fit's factor
    bool in_sharded_fit = false;           // group_eval_run is stamping its members (they all take ONE new fit_id)
    std::vector<nccl_comm_t> comms;        // one per local member (RCCL)
    std::string comm_name;
};

namespace {

int local_index(const gphip_group* g, int rank) {
    for (size_t i = 0; i < g->ranks.size(); ++i)
        if (g->ranks[i] == rank) return (int)i;
    return -1;
}

#define NCCLCHK(call)                                                                             \
    do {                                                                                          \
        int r_ = (call);                                                                          \
        if (r_ != 0) {                                                                            \
            char buf_[512];                                                                       \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, rccl().GetErrorString(r_), __FILE__, __LINE__); \
            h->err = buf_;                                                                        \
            return GPHIP_ERR_HIP;                                                                 \
        }                                                                                         \
    } while (0)

// bytes of the largest (first) outer panel in the packed tile-major layout
size_t group_panel_bytes(const gphip_ctx* m) {
    const int K1 = (int)std::min<int64_t>(m->panel, m->Nt);
    return (size_t)tile_index(K1, K1, (int)m->R) * TS * m->es;
}

int group_member_init(gphip_ctx* h, gphip_ctx* m) {
    // comm stream + three rotating packed-panel buffers (panel k+1 lands while panel k is read; the third
    // keeps the broadcast of k+2 from waiting for REST(k-1)'s readers)
    HIPCHK(hipSetDevice(m->device));
    if (int sr = 0, sw = 0; cu_slice(&sr, &sw)) HIPCHK(make_slice_stream(&m->cstream, sr, sw));      // (developer experiment, see there)
    else HIPCHK(hipStreamCreateWithFlags(&m->cstream, hipStreamNonBlocking));
    // the 8 doubles of the scalar all-reduces exist from the start: a rank must be able to JOIN a collective (with an error
    // flag) even when a later allocation fails -- returning before the all-reduce would leave its peers blocked in RCCL
    HIPCHK(m->dScal8.grow(8 * sizeof(double)));
    // (the three rotating RECEIVE buffers for panels of other ranks are allocated by group_resize_packed when the first
    //  sharded evaluation runs: a handle that only deals batches to its devices never needs them)
    return GPHIP_OK;
}

int group_resize_packed(gphip_ctx* h, gphip_group* g) {      // after "panel" changed
    for (gphip_ctx* m : g->members) {
        bool shared = !g->use_rccl && m->share_local_panels;  // device copies and every rank on this GPU: panels are read in place
        for (gphip_ctx* o : g->members) shared = shared && o->device == m->device;
        const size_t need = (g->replicate != 0 || g->world == 1 || shared) ? 0 : group_panel_bytes(m);   // dense workspace: received in place
        for (Buf& pk : m->packed) {
            if (need <= pk.bytes) continue;
            HIPCHK(hipSetDevice(m->device));
            HIPCHK(pk.grow(need));
        }
    }
    return GPHIP_OK;
}

}  // namespace

static void group_destroy(gphip_ctx* h) {
    gphip_group* g = h->group;
    if (!g) return;
    if (g->use_rccl)
        for (nccl_comm_t c : g->comms)
            if (c) (void)rccl().CommDestroy(c);
    for (size_t i = 1; i < g->members.size(); ++i) gphip_destroy(g->members[i]);
    h->group = nullptr;
    delete g;
}

// devices[i] / ranks[i]: device ordinal and global rank of local member i (nlocal of them); world = ranks of
// the whole job; id128 = RCCL unique id when ranks live in other processes too (nlocal < world).
static int group_create(const void* X, const void* y, int64_t N, int64_t d, int kernel_id, int mean_id, int dtype,
                        const int* devices, const int* ranks, int nlocal, int world, const void* id128, gphip_handle* out) {
    gphip_group* g = new gphip_group;
    g->world = world;
    int rc = GPHIP_OK;
    // (developer experiment GPHIP_CU_PARTITION=1: 2 / 4 / 8 virtual ranks of one device get disjoint slices of its CUs)
    bool partition = false;
    if (const char* e = getenv("GPHIP_CU_PARTITION")) {
        partition = dev_hooks() && !strcmp(e, "1") && !id128 && (nlocal == 2 || nlocal == 4 || nlocal == 8);
        for (int i = 1; i < nlocal; ++i) partition = partition && devices[i] == devices[0];
    }
    for (int i = 0; i < nlocal && rc == GPHIP_OK; ++i) {
        gphip_handle m = nullptr;
        if (partition) { g_slice_r = i; g_slice_w = nlocal; }
        rc = create_ctx(X, y, N, d, kernel_id, mean_id, dtype, devices[i], &m);
        g_slice_w = 0;
        if (rc == GPHIP_OK) {
            g->members.push_back(m);
            g->ranks.push_back(ranks[i]);
        }
    }
    auto bail = [&](int code) {
        if (g->use_rccl)
            for (nccl_comm_t c : g->comms)
                if (c) (void)rccl().CommDestroy(c);
        for (size_t i = 1; i < g->members.size(); ++i) gphip_destroy(g->members[i]);
        if (!g->members.empty()) { g->members[0]->group = nullptr; gphip_destroy(g->members[0]); }
        delete g;
        return code;
    };
    if (id128) {
        // One rank of a multi-process job.  Its peers are entering ncclCommInitRank right now: a rank whose local context
        // could not be created (allocation failure, a covariance function that does not compile HERE, ..) must still join the
        // communicator and say so -- returning first would leave every other rank blocked in RCCL for good.  So: communicator
        // first, then ONE all-reduce of a failure flag; every rank leaves gphip_create*_rank with the same verdict.
        if (!rccl().ok() || nlocal != 1) return bail(GPHIP_ERR_UNSUPPORTED);    // (one device per process in multi-process jobs)
        int dev = devices[0];
        if (dev < 0) (void)hipGetDevice(&dev);
        NcclUniqueId id;
        memcpy(id.internal, id128, sizeof id.internal);
        nccl_comm_t c = nullptr;
        if (hipSetDevice(dev) != hipSuccess || rccl().CommInitRank(&c, world, id, ranks[0]) != 0) return bail(GPHIP_ERR_HIP);
        g->comms.push_back(c);
        g->use_rccl = true;
        g->comm_name = "rccl (ncclCommInitRank, " + rccl().origin + ")";
        Buf dflag;
        double flag = rc != GPHIP_OK ? 1.0 : 0.0, total = -1.0;
        const bool agreed = dflag.grow(sizeof(double)) == hipSuccess &&
                            hipMemcpy(dflag.p, &flag, sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
                            rccl().AllReduce(dflag.p, dflag.p, 1, NCCL_FLOAT64, NCCL_SUM, c, nullptr) == 0 &&
                            hipStreamSynchronize(nullptr) == hipSuccess &&
                            hipMemcpy(&total, dflag.p, sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
        dflag.release();
        if (rc != GPHIP_OK) return bail(rc);
        if (!agreed) return bail(GPHIP_ERR_HIP);
        if (total != 0.0) {
            g_create_error = "another rank of the job could not create its context";
            return bail(GPHIP_ERR_STATE);
        }
    }
    if (rc != GPHIP_OK) return bail(rc);
    gphip_ctx* h = g->members[0];
    for (size_t i = 0; i < g->members.size(); ++i) {
        if (partition) { g_slice_r = (int)i; g_slice_w = nlocal; }
        const int mrc = group_member_init(h, g->members[i]);
        g_slice_w = 0;
        if (mrc != GPHIP_OK) return bail(GPHIP_ERR_HIP);
    }
    // communicator
    bool distinct = true;
    for (int i = 0; i < nlocal; ++i)
        for (int j = 0; j < i; ++j) distinct = distinct && devices[i] != devices[j];
    const char* force = getenv("GPHIP_COMM");
    const bool want_copy = force && !strcmp(force, "copy");
    const bool force_rccl = force && !strcmp(force, "rccl");   // tests: RCCL calls even for virtual ranks sharing a device
    if (id128) {
        // (communicator made above, before the create-status agreement)
    } else if (nlocal > 1 && (distinct || force_rccl) && rccl().ok() && !want_copy) {
        g->comms.assign((size_t)nlocal, nullptr);
        if (rccl().CommInitAll(g->comms.data(), nlocal, devices) != 0) return bail(GPHIP_ERR_HIP);
        g->use_rccl = true;
        g->comm_name = "rccl (ncclCommInitAll, " + rccl().origin + ")";
    } else {
        g->comm_name = "device copies";
    }
    h->group = g;
    *out = h;
    return GPHIP_OK;
}

namespace {

// Where outer panel k lives on local member m during a sharded evaluation: the member's own storage if it owns the
// panel (or keeps the dense workspace: replicate_factor = 1), otherwise one of its three rotating receive buffers.
// Virtual ranks that share a GPU with the owner (device-copy communicator) read the panel where the owner keeps it:
// a factored panel is never written again, so no copy is needed at all.
char* group_panel_ptr(gphip_group* g, int i, int k) {
    gphip_ctx* m = g->members[(size_t)i];
    const int o = k % g->world;
    if (o == g->ranks[(size_t)i] || g->replicate != 0) return dist_panel_range(m, k);
    if (!g->use_rccl && m->share_local_panels) {
        const int lo = local_index(g, o);
        if (lo >= 0 && g->members[(size_t)lo]->device == m->device) return dist_panel_range(g->members[(size_t)lo], k);
    }
    return static_cast<char*>(m->packed[k % 3].p);
}

// Scratch a DRAINING member broadcasts from / into (see group_eval_run): never the panel storage -- a member whose
// gphip_dist_begin failed has no layout (dist_base / dist_adj are void) and its receive buffers may not exist.  One
// allocation of the largest panel's size, kept for the handle's life; null = not even that could be allocated.
char* group_drain_buf(gphip_ctx* m, size_t bytes) {
    if (m->drain_buf.p && m->drain_buf.bytes >= bytes) return static_cast<char*>(m->drain_buf.p);
    for (const Buf& pk : m->packed)
        if (pk.p && pk.bytes >= bytes) return static_cast<char*>(pk.p);
    (void)hipSetDevice(m->device);
    if (m->drain_buf.grow(std::max(bytes, group_panel_bytes(m))) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return static_cast<char*>(m->drain_buf.p);
}

// broadcast panel k (bytes) from rank `root` to every rank, IN PLACE at the root (straight out of its own storage: the
// packed layout makes a panel one contiguous range, nothing is packed); queued on each local member's comm stream,
// which already waits for (a) the receive buffer being free and (b) the owner's factorisation of the panel.
// drain: this process is only keeping its peers' collective sequence alive after a local failure -- same calls, same
// sizes, but every local member sends from / receives into its scratch buffer (the data is void either way).
int group_broadcast(gphip_ctx* h, gphip_group* g, int k, size_t bytes, int root, size_t off = 0, bool drain = false) {
    const int lroot = local_index(g, root);
    if (g->use_rccl) {
        std::vector<char*> bufs(g->members.size(), nullptr);
        for (size_t i = 0; i < g->members.size(); ++i) {
            bufs[i] = drain ? group_drain_buf(g->members[i], bytes) : group_panel_ptr(g, (int)i, k) + off;
            if (!bufs[i]) return fail(h, GPHIP_ERR_HIP, "no memory for the drain buffer of a failed sharded evaluation");
        }
        // Two-hop form (option "bcast_two_hop", part of the agreement check): a receiver of ncclBroadcast is fed over ONE
        // ring, i.e. at one xGMI link's rate while six other links of the fully connected mesh idle.  Here the root scatters
        // piece r of the message to rank r (W - 1 concurrent sends over W - 1 different links, each 1 / W of the bytes) and the
        // ranks then all-gather the pieces in place -- every link of the mesh carries 1 / W of the message at the same time.
        // (At the root the all-gather rewrites its own panel storage with the bytes it already holds.)  The ragged end of a
        // message (< W x 256 bytes) goes out as a plain broadcast.
        const int W = g->world;
        const size_t piece = (g->two_hop && W > 2 && rccl().two_hop_ok()) ? ((bytes / (size_t)W) & ~(size_t)255) : 0;
        if (piece >= 4096) {
            const size_t body = piece * (size_t)W, tail = bytes - body;
            NCCLCHK(rccl().GroupStart());
            for (size_t i = 0; i < g->members.size(); ++i) {
                gphip_ctx* m = g->members[i];
                (void)hipSetDevice(m->device);
                const int ri = g->ranks[i];
                if (ri == root) {
                    for (int r = 0; r < W; ++r)
                        if (r != root) NCCLCHK(rccl().Send(bufs[i] + (size_t)r * piece, piece, NCCL_CHAR, r, g->comms[i], m->cstream));
                } else {
                    NCCLCHK(rccl().Recv(bufs[i] + (size_t)ri * piece, piece, NCCL_CHAR, root, g->comms[i], m->cstream));
                }
            }
            NCCLCHK(rccl().GroupEnd());
            NCCLCHK(rccl().GroupStart());
            for (size_t i = 0; i < g->members.size(); ++i) {
                gphip_ctx* m = g->members[i];
                (void)hipSetDevice(m->device);
                NCCLCHK(rccl().AllGather(bufs[i] + (size_t)g->ranks[i] * piece, bufs[i], piece, NCCL_CHAR, g->comms[i], m->cstream));
            }
            NCCLCHK(rccl().GroupEnd());
            if (tail) {
                NCCLCHK(rccl().GroupStart());
                for (size_t i = 0; i < g->members.size(); ++i) {
                    gphip_ctx* m = g->members[i];
                    (void)hipSetDevice(m->device);
                    NCCLCHK(rccl().Broadcast(bufs[i] + body, bufs[i] + body, tail, NCCL_CHAR, root, g->comms[i], m->cstream));
                }
                NCCLCHK(rccl().GroupEnd());
            }
            return GPHIP_OK;
        }
        NCCLCHK(rccl().GroupStart());
        for (size_t i = 0; i < g->members.size(); ++i) {
            gphip_ctx* m = g->members[i];
            (void)hipSetDevice(m->device);
            NCCLCHK(rccl().Broadcast(bufs[i], bufs[i], bytes, NCCL_CHAR, root, g->comms[i], m->cstream));
        }
        NCCLCHK(rccl().GroupEnd());
        return GPHIP_OK;
    }
    if (drain) return GPHIP_OK;                             // device copies: every rank is local, nobody else is waiting
    if (lroot < 0) return fail(h, GPHIP_ERR_STATE, "copy communicator needs every rank in this process");
    gphip_ctx* src = g->members[(size_t)lroot];
    const char* from = group_panel_ptr(g, lroot, k) + off;
    for (size_t i = 0; i < g->members.size(); ++i) {
        gphip_ctx* m = g->members[i];
        if (m == src) continue;
        HIPCHK(hipSetDevice(m->device));
        char* to = group_panel_ptr(g, (int)i, k) + off;
        if (to == from) continue;                           // same GPU as the owner: the panel is read in place
        if (m->device == src->device) HIPCHK(hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToDevice, m->cstream));
        else HIPCHK(hipMemcpyPeerAsync(to, m->device, from, src->device, bytes, m->cstream));
    }
    return GPHIP_OK;
}

// Ranks in other processes: make sure every rank is about to run the SAME schedule (a different panel width means different
// message sizes: RCCL would hang or corrupt) and tell everybody when somebody cannot.  Two tiny all-reduces over one 8-double
// buffer: MAX over (x_0, x_1, x_2, -x_0, -x_1, -x_2) -- the ranks agree on entry i iff max(x_i) == -max(-x_i), an exact
// comparison whatever the values -- and SUM over the count of ranks already in trouble (a rank that cannot even upload sends
// NaN there, which a sum propagates).  Returns the same verdict on every rank.
int group_agree(gphip_ctx* h, gphip_group* g, const double* mine, int n, const char* what) {
    if ((int)g->members.size() == g->world && !(g->use_rccl && g->world == 1)) return GPHIP_OK;     // everybody is local
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};                // [0..2] x, [3..5] -x, [6] ranks that are already in trouble
    for (int i = 0; i < n && i < 3; ++i) { v[i] = mine[i]; v[3 + i] = -mine[i]; }
    // Nothing rank-local may make this rank skip the all-reduces (its peers are about to enter them): a rank in trouble says so
    // in v[6] (or, if it cannot even upload, sends NaN), and EVERY rank then returns GPHIP_ERR_HIP from this call.
    bool sick = hipSetDevice(h->device) != hipSuccess;
    if (!h->dScal8.p) return fail(h, GPHIP_ERR_HIP, "scalar buffer of the multi-device handle is missing");
    if (h->debug_fail_hip > 0 && --h->debug_fail_hip == 0) sick = true;                               // fault injection (tests)
    if (sick) v[6] = 1.0;
    if (hipMemcpyAsync(h->dScal8.p, v, sizeof v, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
        (void)hipGetLastError();
        sick = true;
        (void)hipMemsetAsync(h->dScal8.p, 0xff, sizeof v, h->stream);                                   // all-ones bytes = NaN
    }
    if (rccl().AllReduce(h->dScal8.p, h->dScal8.p, 6, NCCL_FLOAT64, NCCL_MAX, g->comms[0], h->stream) != 0 ||
        rccl().AllReduce(h->dScal8.as<double>() + 6, h->dScal8.as<double>() + 6, 2, NCCL_FLOAT64, NCCL_SUM, g->comms[0], h->stream) != 0) {
        g->broken = true;
        return fail(h, GPHIP_ERR_HIP, "ncclAllReduce of the configuration check failed");
    }
    if (hipMemcpyAsync(v, h->dScal8.p, sizeof v, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
        (void)hipGetLastError();
        g->broken = true;                                  // this rank cannot learn the verdict its peers act on
        return fail(h, GPHIP_ERR_HIP, "reading back the configuration check failed");
    }
    if (!(v[6] == 0.0))
        return fail(h, GPHIP_ERR_HIP, sick ? "this rank failed before the configuration check of a sharded evaluation"
                                           : "another rank of the job failed before the configuration check of a sharded evaluation");
    for (int i = 0; i < n && i < 3; ++i)
        if (!(v[i] == -v[3 + i])) {                        // max != min
            char buf[256];
            snprintf(buf, sizeof buf, "the ranks of this job disagree on %s (entry %d): every rank must use the same value", what, i);
            h->err = buf;
            return GPHIP_ERR_ARG;
        }
    return GPHIP_OK;
}

// One likelihood evaluation factored by all ranks of the group together.  keep: leave the factor (each rank: its own
// panels; with replicate_factor = 1 all of it), z and the block inverses in place (fit).  Results identical on every rank.
//
// Failure semantics: a rank-local failure of a COMPUTE step (launch error, bad state) does not leave the other ranks
// blocked inside RCCL -- the failing rank keeps issuing the remaining broadcasts (of data nobody will use) and the final
// all-reduce, which carries an error count, so every rank of the job returns GPHIP_ERR_HIP from the same call.  A failure
// of a collective call itself is fatal for the communicator: the call returns at once and the handle refuses further
// sharded evaluations (GPHIP_ERR_STATE).
int group_eval_run(gphip_ctx* h, const double* theta, int p, bool keep, double* out, double* parts, int* info) {
    gphip_group* g = h->group;
    const int nl = (int)g->members.size(), W = g->world;
    if (p != h->p) return fail(h, GPHIP_ERR_DIM, "theta has the wrong length for this kernel/mean");
    if (g->broken) return fail(h, GPHIP_ERR_STATE, "a collective call failed earlier: this multi-device handle can no longer shard");
    int nouter = 0;
    int rc = gphip_dist_num_panels(h, &nouter);
    if (rc) return rc;
    // the broadcast form resolved: an explicit 0 / 1, or by the size of the job (a receiver of ncclBroadcast is fed over ONE link;
    // from four ranks on the all-links form is what the schedule's own model needs, profiles/r06_scale_model.txt)
    const bool two_hop = h->bcast_two_hop < 0 ? (W >= 4 && g->use_rccl && rccl().two_hop_ok()) : h->bcast_two_hop != 0;
    {
        const double cfg[3] = {(double)h->panel, (double)h->N,
                               (double)((keep ? 1 : 0) + 2 * (h->replicate_factor != 0 ? 1 : 0) + 4 * (h->bcast_chunks ? 1 : 0) +
                                        8 * (two_hop ? 1 : 0))};
        rc = group_agree(h, g, cfg, 3, "panel / N / (fit-vs-likelihood, replicate_factor, bcast_chunks, bcast_two_hop)");
        if (rc) return rc;
    }
    // From here to the final all-reduce this rank is inside a COLLECTIVE SEQUENCE (nouter x nchunks broadcasts, one
    // all-reduce) that its peers will issue whatever happens here.  So nothing rank-local returns early any more: a failed
    // HIP call / compute step / allocation switches the process to DRAIN mode -- no further compute, the remaining
    // broadcasts go through a scratch buffer (never through panel storage, whose layout may not exist), and the final
    // all-reduce carries the error count, so EVERY rank returns the error from this same call.  Only a failing
    // collective call itself ends the sequence (the communicator is then unusable: g->broken).
    g->replicate = h->replicate_factor;
    g->two_hop = two_hop;
    const auto t_issue0 = std::chrono::steady_clock::now();
    int failed = GPHIP_OK;                                  // first local failure (drain mode)
    std::string failed_why;
    auto compute = [&](gphip_ctx* m, int code) {            // surface a member's error text; switch to drain mode
        if (code != GPHIP_OK && failed == GPHIP_OK) { failed = code; failed_why = m->err; }
    };
    auto soft = [&](hipError_t e, const char* what) {       // a HIP call of the schedule itself
        if (h->debug_fail_hip > 0 && --h->debug_fail_hip == 0) e = hipErrorUnknown;                  // fault injection (tests)
        if (e != hipSuccess && failed == GPHIP_OK) {
            (void)hipGetLastError();
            failed = GPHIP_ERR_HIP;
            failed_why = std::string(what) + " failed in a sharded evaluation: " + hipGetErrorString(e);
        }
        return e == hipSuccess;
    };
#define SOFT(call) soft((call), #call)
    compute(h, group_resize_packed(h, g));
    std::vector<std::vector<hipEvent_t>> ev_rest((size_t)nl, std::vector<hipEvent_t>((size_t)nouter + 1, nullptr));
    std::vector<std::vector<hipEvent_t>> ev_bcast = ev_rest;
    // REST(k) on owner(k + 2) is issued in two pieces: the columns of outer panel k + 2 first (own event), then the remainder.
    // LA(k + 1) -- the next step of the owner chain factor -> broadcast -> look-ahead update -> factor -- needs only the
    // former, so the rest of that rank's trailing share is off the chain (it used to wait for ALL of REST(k)).
    std::vector<std::vector<hipEvent_t>> ev_first = ev_rest;
    auto owner = [&](int k) { return k % W; };
    // "dist_owner_yield": while a rank factors its panel, its own trailing updates stand back -- by EVENTS, not by stream priority.
    // A panel launch that becomes ready while a trailing GEMM of the same GPU is running gets its workgroups placed only as that
    // launch runs out of its own (a CU hands a freed slot to the next workgroup of the launch it is already dispatching, whatever
    // the priorities of the streams: EXPERIMENTS.md round 3, and scripts/gpu_cu_partition.py round 6: ranks that really run side
    // by side scaled 1.6x / 2.2x / 2.0x on 2 / 4 / 8 slices).  So: on owner(k + 1) the remainder of REST(k - 1) and REST(k) are
    // queued BEHIND factor(k + 1)'s end event; only the piece of REST(k - 1) that panel k + 1 itself needs runs before it.
    // Default: from 4 ranks on, where the chain is what bounds the evaluation (2 ranks are bound by their trailing work, and
    // whatever order a GPU does its work in costs the same).
    const bool yield = W > 1 && (h->dist_owner_yield < 0 ? W >= 4 : h->dist_owner_yield != 0);
    std::vector<hipEvent_t> ev_fact((size_t)nouter + 1, nullptr);     // end of factor(k) on its owner's panel stream (local owners)
    std::vector<int> deferred((size_t)nl, -1);                         // member i: step whose REST remainder is still to be issued
    auto comm_fatal = [&](int code) { g->broken = true; return code; };
    auto wait_on = [&](hipStream_t st, hipEvent_t ev) { if (ev && failed == GPHIP_OK) SOFT(hipStreamWaitEvent(st, ev, 0)); };
    auto record = [&](gphip_ctx* m, hipStream_t st) -> hipEvent_t {
        if (failed != GPHIP_OK) return nullptr;
        hipEvent_t ev = sync_event(m);
        return (ev && SOFT(hipEventRecord(ev, st))) ? ev : nullptr;
    };

    // owner factors panel k (its panel stream); every rank receives it (comm streams)
    auto factor_and_broadcast = [&](int k) -> int {
        const int o = owner(k), lo = local_index(g, o);
        hipEvent_t factored = nullptr;
        std::vector<hipEvent_t> colev;                                 // owner: "tile column s of the panel is final"
        std::vector<std::pair<unsigned int*, unsigned int>> colw;      // .. or, from inside a dataflow panel launch (dist_panel_df = 3):
                                                                       // (counter address, value it reaches when the column is final)
        if (lo >= 0 && failed == GPHIP_OK) {
            gphip_ctx* m = g->members[(size_t)lo];
            {
                Scoped<decltype(m->col_events)> ev(m->col_events, h->bcast_chunks ? &colev : nullptr);
                Scoped<decltype(m->col_waits)> cw(m->col_waits, h->bcast_chunks ? &colw : nullptr);
                compute(m, gphip_dist_factor_panel(m, k, nullptr));
            }
            SOFT(hipSetDevice(m->device));
            factored = record(m, m->pstream);
            ev_fact[(size_t)k] = factored;
        }
        // The panel goes out ONE TILE COLUMN AT A TIME ("bcast_chunks", default on; every rank issues the same broadcasts --
        // the setting is part of the agreement check): a tile column is final after its own solve, so columns 0 .. nin-2 travel
        // while the owner still factors the rest of the panel, and only the last, shortest column's transfer stays on the
        // chain owner(k) -> broadcast -> LA(k) on owner(k+1).  (A tile column is one contiguous range of the tile-major layout.)
        const int P0 = h->panel * k, nin = (int)std::min<int64_t>(h->panel, h->Nt - P0);
        const int nchunks = h->bcast_chunks ? nin : 1;
        size_t off = 0;
        for (int s = 0; s < nchunks; ++s) {
            const size_t bytes = nchunks == 1 ? (size_t)dist_panel_tiles(h, k) * TS * h->es
                                              : (size_t)(h->R - (P0 + s)) * TS * h->es;
            hipEvent_t ready = (nchunks > 1 && (int)colev.size() == nin) ? colev[(size_t)s] : factored;
            // a column of a dataflow panel launch that is final BEFORE the launch ends (all but the last one): a stream-ordered wait
            // on its tile counter instead of the launch's end event.  Only streams of the owner's own device wait on the counter.
            const bool by_count = nchunks > 1 && (int)colw.size() == nin && s + 1 < nin && lo >= 0;
            for (int i = 0; i < nl && failed == GPHIP_OK; ++i) {
                gphip_ctx* m = g->members[(size_t)i];
                SOFT(hipSetDevice(m->device));
                if (s == 0 && k >= 3) wait_on(m->cstream, ev_rest[(size_t)i][(size_t)k - 3]);   // REST(k-3) was the receive buffer's last reader
                if (i == lo || !g->use_rccl) {                             // copies read the owner's storage directly
                    if (by_count && m->device == g->members[(size_t)lo]->device)
                        SOFT(hipStreamWaitValue32(m->cstream, colw[(size_t)s].first, colw[(size_t)s].second, hipStreamWaitValueGte, 0xFFFFFFFFu));
                    else
                        wait_on(m->cstream, ready);
                }
            }
            const int c = group_broadcast(h, g, k, bytes, o, off, failed != GPHIP_OK);
            if (c) return comm_fatal(c);
            off += bytes;
        }
        for (int i = 0; i < nl && failed == GPHIP_OK; ++i) {
            gphip_ctx* m = g->members[(size_t)i];
            SOFT(hipSetDevice(m->device));
            ev_bcast[(size_t)i][(size_t)k] = record(m, m->cstream);
        }
        return GPHIP_OK;
    };

    for (int i = 0; i < nl; ++i) {
        gphip_ctx* m = g->members[(size_t)i];
        m->sync_used = 0;
        if (m != h) {                                                  // same options / point-dependent arrays on every member
            m->replicate_factor = h->replicate_factor;
            m->pw_mean_host = h->pw_mean_host; m->pw_nug_host = h->pw_nug_host;
        }
        if (failed == GPHIP_OK) compute(m, gphip_dist_begin(m, theta, p, g->ranks[(size_t)i], W));
        if (m != h) m->pw_mean_host = m->pw_nug_host = nullptr;
        if (failed != GPHIP_OK) continue;
        SOFT(hipSetDevice(m->device));
        hipEvent_t built = record(m, m->stream);
        wait_on(m->pstream, built);
        wait_on(m->cstream, built);                                    // (with replicate_factor = 1 panels land in the workspace)
    }
    rc = factor_and_broadcast(0);
    if (rc) return rc;
    for (int k = 0; k < nouter; ++k) {
        if (k + 1 < nouter) {
            const int lo = local_index(g, owner(k + 1));
            if (lo >= 0 && failed == GPHIP_OK) {                       // LA(k) on the next owner's panel stream
                gphip_ctx* m = g->members[(size_t)lo];
                SOFT(hipSetDevice(m->device));
                wait_on(m->pstream, ev_bcast[(size_t)lo][(size_t)k]);
                if (k >= 1) wait_on(m->pstream, ev_first[(size_t)lo][(size_t)k - 1]);      // REST(k-1)'s piece on panel k + 1
                if (failed == GPHIP_OK) compute(m, gphip_dist_update(m, k, group_panel_ptr(g, lo, k), k + 1, k + 2, 1));
            }
            rc = factor_and_broadcast(k + 1);
            if (rc) return rc;
        }
        for (int i = 0; i < nl && failed == GPHIP_OK; ++i) {           // REST(k) on everyone's main stream
            gphip_ctx* m = g->members[(size_t)i];
            SOFT(hipSetDevice(m->device));
            if (yield && k + 1 < nouter && g->ranks[(size_t)i] == owner(k + 1)) {
                wait_on(m->stream, ev_fact[(size_t)k + 1]);            // this rank is factoring panel k + 1: trailing work after it
                if (k >= 1 && deferred[(size_t)i] == k - 1 && failed == GPHIP_OK) {
                    compute(m, gphip_dist_update(m, k - 1, group_panel_ptr(g, i, k - 1), k + 2, nouter + 1, 0));
                    ev_rest[(size_t)i][(size_t)k - 1] = record(m, m->stream);
                    deferred[(size_t)i] = -1;
                }
            }
            wait_on(m->stream, ev_bcast[(size_t)i][(size_t)k]);
            // (the last panel has no look-ahead step: its REST starts at the corner tile)
            int first = k + 1 < nouter ? k + 2 : k + 1;
            bool defer = false;
            if (W > 1 && k + 2 < nouter && g->ranks[(size_t)i] == owner(k + 2) && failed == GPHIP_OK) {
                compute(m, gphip_dist_update(m, k, group_panel_ptr(g, i, k), k + 2, k + 3, 0));
                ev_first[(size_t)i][(size_t)k] = record(m, m->stream);
                first = k + 3;
                defer = yield;                                         // the remainder goes out behind factor(k + 2), next step
            }
            if (defer) {
                deferred[(size_t)i] = k;
                continue;
            }
            if (failed == GPHIP_OK)
                compute(m, gphip_dist_update(m, k, group_panel_ptr(g, i, k), first, nouter + 1, 0));
            ev_rest[(size_t)i][(size_t)k] = record(m, m->stream);
            if (!ev_first[(size_t)i][(size_t)k]) ev_first[(size_t)i][(size_t)k] = ev_rest[(size_t)i][(size_t)k];
        }
    }
    // host time this thread spent ISSUING the schedule (every launch, event and collective call of all local ranks), before it
    // first blocks: read-only option "last_issue_us" (scripts/gpu_multi_overhead.py, the host term of scripts/scale_model.py)
    h->last_issue_us = (int)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_issue0).count();
    double vals[8] = {0, 0, 0, 0, 0, 0, 0, 0};                         // log det, quad, #not-SPD, #NaN, #failed ranks
    for (int i = 0; i < nl; ++i) {
        gphip_ctx* m = g->members[(size_t)i];
        (void)hipSetDevice(m->device);
        if (hipStreamSynchronize(m->cstream) != hipSuccess) SOFT(hipErrorUnknown);
        double ld = 0, qd = 0;
        int inf = 0;
        if (m->dist_world > 0 && failed == GPHIP_OK) compute(m, gphip_dist_end(m, &ld, &qd, &inf));    // syncs panel + main streams
        vals[0] += ld; vals[1] += qd;
        vals[2] += inf == GPHIP_INFO_NOT_SPD; vals[3] += inf == GPHIP_INFO_NAN;
    }
    vals[4] = failed != GPHIP_OK ? 1.0 : 0.0;
    if (nl < W || (g->use_rccl && W == 1)) {                           // ranks elsewhere: one tiny all-reduce
        (void)hipSetDevice(h->device);
        if (!h->dScal8.p) return comm_fatal(fail(h, GPHIP_ERR_HIP, "scalar buffer of the multi-device handle is missing"));
        if (hipMemcpyAsync(h->dScal8.p, vals, sizeof vals, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
            // cannot even upload the error count: send a poisoned vector (NaN in every entry reads as "somebody failed")
            (void)hipGetLastError();
            if (failed == GPHIP_OK) { failed = GPHIP_ERR_HIP; failed_why = "uploading the scalars of a sharded evaluation failed"; }
            (void)hipMemsetAsync(h->dScal8.p, 0xff, sizeof vals, h->stream);
        }
        if (rccl().AllReduce(h->dScal8.p, h->dScal8.p, 8, NCCL_FLOAT64, NCCL_SUM, g->comms[0], h->stream) != 0)
            return comm_fatal(fail(h, GPHIP_ERR_HIP, "ncclAllReduce of the scalars failed"));
        if (hipMemcpyAsync(vals, h->dScal8.p, sizeof vals, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess) {
            (void)hipGetLastError();
            return comm_fatal(fail(h, GPHIP_ERR_HIP, "reading back the scalars of a sharded evaluation failed"));
        }
    }
#undef SOFT
    if (!(vals[4] == 0)) {                                             // somebody failed (or sent NaN): every rank reports it
        h->err = failed != GPHIP_OK ? failed_why : std::string("another rank of the job failed in this sharded evaluation");
        return failed != GPHIP_OK ? failed : GPHIP_ERR_HIP;
    }
    const double logdet = vals[0], quad = vals[1];
    const double ll = -0.5 * ((double)h->N * LOG_TWO_PI + logdet + quad);
    int inf = vals[3] > 0 ? GPHIP_INFO_NAN : (vals[2] > 0 ? GPHIP_INFO_NOT_SPD : GPHIP_INFO_OK);
    if (inf == 0 && !std::isfinite(ll)) inf = GPHIP_INFO_NAN;
    *info = inf;
    *out = ll;
    if (parts) { parts[0] = logdet; parts[1] = quad; }
    for (gphip_ctx* m : g->members) { invalidate_fit(m); m->null_fit = false; }
    if (keep && inf == 0) {
        ++g->fit_id;
        g->in_sharded_fit = true;
        // The factor stays where it is: every rank holds its own panels (L, z in the rhs tile row, the 128-block inverses
        // of its diagonal blocks) -- or, with replicate_factor = 1, everything (then the inverses of the received diagonal
        // blocks are rebuilt locally).
        for (size_t i = 0; i < g->members.size(); ++i) {
            gphip_ctx* m = g->members[i];
            HIPCHK(hipSetDevice(m->device));
            if (g->replicate != 0) {
                if (m->dtype == 64)
                    hipLaunchKernelGGL(trtri128_kernel<double>, dim3((unsigned)m->Nt, 1), dim3(256), potrf_lds<double>(), m->stream,
                                       (const double*)m->dA.p, (long)m->slot_elems, (double*)m->dW.p, (int)m->Nt, 0);
                else
                    hipLaunchKernelGGL(trtri128_kernel<float>, dim3((unsigned)m->Nt, 1), dim3(256), potrf_lds<float>(), m->stream,
                                       (const float*)m->dA.p, (long)m->slot_elems, (float*)m->dW.p, (int)m->Nt, 0);
                HIPCHK(hipStreamSynchronize(m->stream));
                HIPCHK(hipGetLastError());
            }
            if (g->replicate == 0 && m->dist_df_active) {
                // dataflow panels leave inverses of 64-blocks behind: rebuild the 128-block inverses of the OWNED panels (the
                // streamed prediction substitutes with them; received panels are rebuilt on arrival there anyway)
                int npan = 0;
                (void)gphip_dist_num_panels(m, &npan);
                for (int k = g->ranks[i]; k < npan; k += W) {
                    const int K0 = k * m->panel, K1 = (int)std::min<int64_t>(K0 + m->panel, m->Nt);
                    hipLaunchKernelGGL(trtri128_kernel<double>, dim3((unsigned)(K1 - K0), 1), dim3(256), potrf_lds<double>(), m->stream,
                                       (const double*)dist_panel_base(m, k), 0l, (double*)m->dW.p, (int)m->Nt, K0);
                }
                HIPCHK(hipStreamSynchronize(m->stream));
                HIPCHK(hipGetLastError());
            }
            record_fit(m, true, theta, p, logdet);
            m->fit_id = g->fit_id;
            m->dist_fit = g->replicate == 0;
            m->shard_fit = true;
            m->fit_rank = g->ranks[i]; m->fit_world = W;
        }
        g->in_sharded_fit = false;
    }
    return GPHIP_OK;
}

// the schedule with its failure path: whatever went wrong (HIP / RCCL error, bad argument), every local member is
// drained and taken out of "distributed" mode, so the handle stays usable and nothing is left queued on buffers the
// next call reuses
int group_eval(gphip_ctx* h, const double* theta, int p, bool keep, double* out, double* parts, int* info) {
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    const int rc = group_eval_run(h, theta, p, keep, out, parts, info);
    if (rc != GPHIP_OK) {
        const std::string why = h->err;
        for (gphip_ctx* m : h->group->members) {
            (void)hipSetDevice(m->device);
            (void)hipStreamSynchronize(m->cstream);
            (void)hipStreamSynchronize(m->pstream);
            (void)hipStreamSynchronize(m->stream);
            (void)hipGetLastError();
            m->dist_world = 0; m->dist_rank = 0;
            invalidate_fit(m);
        }
        h->err = why;
    }
    return rc;
}

bool group_shards(const gphip_ctx* h) {
    // shard_min_n = 0 forces the sharded schedule even for a world of one (tests of the RCCL binding on one GPU)
    if (!h->group || h->kernel_id == GPHIP_KERNEL_NULL) return false;
    return h->shard_min_n <= 0 || (h->group->world > 1 && h->N >= h->shard_min_n);
}

// run f(member index) on one host thread per local member; first non-zero status wins
template <typename F>
int group_parallel(gphip_ctx* h, F f) {
    gphip_group* g = h->group;
    const int nl = (int)g->members.size();
    std::vector<int> rcs((size_t)nl, GPHIP_OK);
    std::vector<std::thread> ts;
    for (int i = 1; i < nl; ++i) ts.emplace_back([&, i] { rcs[(size_t)i] = f(i); });
    rcs[0] = f(0);
    for (auto& t : ts) t.join();
    for (int i = 0; i < nl; ++i)
        if (rcs[(size_t)i] != GPHIP_OK) {
            if (i > 0) h->err = g->members[(size_t)i]->err;
            return rcs[(size_t)i];
        }
    return GPHIP_OK;
}

// axis (1): contiguous blocks of theta to the local devices, no collective
int group_eval_batch(gphip_ctx* h, const double* Theta, int B, int p, double* out, double* parts, int* info) {
    gphip_group* g = h->group;
    const int nl = (int)g->members.size();
    if (nl == 1 || B < 2) return eval_batch_local(h, Theta, B, p, out, parts, info);
    const double *pm = h->pw_mean_host, *pn = h->pw_nug_host;
    return group_parallel(h, [&](int i) {
        const int b0 = (int)((long)B * i / nl), b1 = (int)((long)B * (i + 1) / nl);
        if (b1 <= b0) return (int)GPHIP_OK;
        gphip_ctx* m = g->members[(size_t)i];
        if (m != h) {                                                      // the member's rows of the point-dependent arrays
            m->pw_mean_host = pm ? pm + (size_t)b0 * h->N : nullptr;
            m->pw_nug_host = pn ? pn + (size_t)b0 * h->N : nullptr;
        }
        const int c = eval_batch_local(m, Theta + (size_t)b0 * p, b1 - b0, p, out + b0, parts ? parts + 2 * b0 : nullptr, info + b0);
        if (m != h) m->pw_mean_host = m->pw_nug_host = nullptr;
        return c;
    });
}

}  // namespace
