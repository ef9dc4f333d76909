"""Static guards on the HIP host code for bug classes that tests hit only by luck.

1. Null-stream memory operations.  Every handle works on its own NON-BLOCKING streams, which are not ordered with the
   null stream: a `hipMemset(...)` / `hipMemcpy(...)` of device memory that kernels on those streams read next is a
   race (round 2: the flag / ticket clears after a slot re-allocation -- wrong likelihoods and memory faults once per
   few thousand handles, found by scripts/gpu_api_fuzz.py).  Device memory is cleared / copied with the *Async forms
   on the handle's stream (create_ctx's uploads too: stream-ordered, then a stream synchronise).
2. No CUDA compatibility layer, no multi-backend dispatch (the build is gfx950-only by contract)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesianinference_amd", "csrc")


def _code(path):
    text = open(path).read()
    text = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_no_null_stream_memory_operations_on_device_buffers():
    bad = []
    for name in ("gphip.hip", "gphip_multi.inc", "gp_kernels.h"):
        code = _code(os.path.join(CSRC, name))
        for m in re.finditer(r"\bhip(Memset|Memcpy|Memcpy2D|MemsetD8|MemsetD32)\s*\(([^;]*)\)\s*[;)]", code):
            call = re.sub(r"\s+", " ", m.group(0)).rstrip(";)").rstrip() + ")"
            call = call if call.count("(") == call.count(")") else call[:-1]
            bad.append((name, call[:100]))
    assert not bad, bad


def test_device_and_pinned_memory_only_through_the_owning_buffer_type():
    # every allocation / free of the host code sits inside `struct Buf` (gphip.hip): a buffer knows its size and frees
    # itself, so no hand-written free list can miss one and no size field can disagree with its pointer
    call = re.compile(r"\bhip\w*(Malloc|Free)\w*")
    gphip = _code(os.path.join(CSRC, "gphip.hip"))
    buf = re.search(r"\nstruct Buf \{.*?\n\};", gphip, flags=re.S)
    assert buf and call.search(buf.group(0)), "the owning buffer type (struct Buf) is missing from gphip.hip"
    sources = {"gphip.hip": gphip[:buf.start()] + gphip[buf.end():]}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(".inc"):
            sources[name] = _code(os.path.join(CSRC, name))
    bad = [(name, line.strip()) for name, code in sources.items() for line in code.splitlines() if call.search(line)]
    assert not bad, bad


def test_factorisation_mode_flags_only_through_the_scope_type():
    # want_w / want_u tell the next factorisation what to leave behind; a caller that set them by hand had to clear them on
    # every exit path, and one that returned early left every later evaluation on the handle in the wrong mode.  `struct
    # FactorMode` (gphip.hip) sets them and restores them in its destructor; nothing else assigns them.
    assign = re.compile(r"\bwant_[wu]\s*[|&^]?=(?!=)")
    gphip = _code(os.path.join(CSRC, "gphip.hip"))
    scope = re.search(r"\nstruct FactorMode \{.*?\n\};", gphip, flags=re.S)
    assert scope and assign.search(scope.group(0)), "the scope type (struct FactorMode) is missing from gphip.hip"
    sources = {"gphip.hip": gphip[:scope.start()] + gphip[scope.end():]}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(".inc"):
            sources[name] = _code(os.path.join(CSRC, name))
    # (the context's own member initialisers `bool want_w = false;` are declarations, not assignments by a caller)
    bad = [(name, line.strip()) for name, code in sources.items() for line in code.splitlines()
           if assign.search(line) and not re.match(r"\s*bool want_[wu] = false;", line)]
    assert not bad, bad


def test_targeted_stream_changes_only_through_a_scope():
    # `cs`, the stream the launch helpers queue on, rests at the main stream: it is assigned where a context's streams are made
    # (create_ctx) and in gphip_set_streams, and retargeted only through `Scoped<hipStream_t>`, which puts it back on every exit
    # path.  A by-hand `h->cs = h->pstream` that an early return skipped left every later call on the panel stream; the main
    # stream itself is never swapped for another.
    hits = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".inc", ".hip")):
            code = _code(os.path.join(CSRC, name))
            hits[name] = (len(re.findall(r"->cs\s*=(?!=)", code)), len(re.findall(r"->stream\s*=(?!=)", code)))
    assert hits.pop("gphip.hip") == (2, 1), "cs: create_ctx + gphip_set_streams; stream: gphip_set_streams"
    assert all(v == (0, 0) for v in hits.values()), hits
    assert "Scoped<hipStream_t>" in _code(os.path.join(CSRC, "gphip.hip"))


def test_sparse_bound_has_one_forward_pass_and_owned_phase_records():
    # The collapsed bound's forward pass exists once, in the group evaluator the one-theta and the batched entry points share
    # (DESIGN.md section 8f): a second copy of the chunk loop or of the formula for F drifts.  Phases are named by the
    # SparsePhaseId enum, and the HIP-event records of a call belong to `struct SparsePhases`, whose destructor hands the
    # events back to the pool on every exit path: nothing else harvests them.
    code = _code(os.path.join(CSRC, "gphip_sparse.inc"))
    for fn in ("sparse_queue_accumulate", "sparse_queue_diag"):
        uses = re.findall(r"\b%s\b.{0,24}" % fn, code)              # its definition `int fn(gphip_sparse_ctx* h, ..` and its call sites
        sites = [u for u in uses if not u.startswith(fn + "(gphip_sparse_ctx*")]
        assert len(uses) == 2 and len(sites) == 1, (fn, uses)
    assert len(re.findall(r"\bsparse_blocksum_kernel\b", code)) == 1          # (defined in gp_sparse.h)
    assert len(re.findall(r"\bLOG_TWO_PI\b", code)) == 1
    scopes = re.findall(r"\bSparseScope\s+\w+\s*\(([^;]*)\);", code)
    assert len(scopes) >= 15, scopes
    for args in scopes:                                              # (owner, phase, stream)
        assert re.fullmatch(r"PH_[A-Z_]+", args.split(",")[1].strip()), args
    owner = re.search(r"\nstruct SparsePhases \{.*?\n\};", code, flags=re.S)
    assert owner and "~SparsePhases() { harvest(); }" in owner.group(0), "the owner of the phase records (struct SparsePhases) is missing"
    rest = code[:owner.start()] + code[owner.end():]
    assert "sparse_harvest" not in rest
    assert all(re.fullmatch(r"\w+\.harvest\(\)", m) for m in re.findall(r"[\w.>-]*\bharvest\b(?:\(\))?", rest)), "harvest outside the owner"


def test_sparse_prediction_pass_and_chunk_head_exist_once():
    # Prediction from a sparse object is one pass (sparse_predict_pass: the one-theta call and the call over samples are its two
    # callers) and a chunk of data points has one head (sparse_chunk_head: the group evaluator and the gradient's recomputed
    # chunks), DESIGN.md sections 8d and 8h.  What they share with the exact path belongs to the exact path: the strip rule, the
    # launch of predict_partial_kernel and the choice between the dataflow launch and the batched GEMM substitution.
    host = {name: _code(os.path.join(CSRC, name)) for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".inc"))}
    everything = "\n".join(host.values())
    assert len(re.findall(r"\bpredict_partial_kernel\b", everything)) == 1               # (defined in gp_kernels.h)
    assert len(re.findall(r"hipLaunchKernelGGL\(\s*predict_partial_kernel\b", host["gphip.hip"])) == 1
    assert len(re.findall(r"2048 \+", everything)) == 1                                  # the strip rule's literal
    assert len(re.findall(r"\bsamples_forward_df\(", everything)) == 2                   # its definition and one call
    code = host["gphip_sparse.inc"]
    assert len(re.findall(r"\bsparse_predict_finish_kernel\b", code)) == 1               # (defined in gp_sparse.h)
    for fn in ("sparse_stage_test_arrays", "sparse_queue_handover", "sparse_queue_resid", "sparse_queue_resid_pw"):
        uses = re.findall(r"\b%s\b.{0,24}" % fn, code)              # its definition `int fn(gphip_sparse_ctx* h, ..` and its call sites
        sites = [u for u in uses if not u.startswith(fn + "(gphip_sparse_ctx*")]
        assert len(uses) == 2 and len(sites) == 1, (fn, uses)
    for gone in ("sparse_partial_strips", "sparse_queue_partial", "sparse_queue_forward"):
        assert gone not in everything, gone


def test_strip_split_contraction_exists_once():
    # The joint downdate and the sparse accumulation are one device algorithm (gp_contract.h): tile-list
    # decode, thin-tile rule, two-stage software pipeline and the reduction of the strip partials.  A hand copy in a caller's
    # header means every fix to the barrier / wait placement or to the thin-tile rule has to be made and proved twice.
    joint, sparse, contract = (_code(os.path.join(CSRC, n)) for n in ("gp_joint.h", "gp_sparse.h", "gp_contract.h"))
    thin = (r"\bi\s*>=\s*16\b", r"\bj\s*>=\s*64\b")           # the reduce kernel's skip conditions
    for code in (joint, sparse):
        assert "sched_barrier" not in code and "pin_frags" not in code
        assert "tri_decode" not in code
        assert not any(re.search(t, code) for t in thin)
    assert all(len(re.findall(t, contract)) == 1 for t in thin)
    assert len(re.findall(r"__global__[^;{]*\bvoid\s+\w*reduce_kernel\b", joint + sparse)) == 0
    # the two entry kernels are its only users: downdate_kernel calls it on either side of `if constexpr (SEG)`
    users = {name: len(re.findall(r"\bstrip_contract\b", _code(os.path.join(CSRC, name)))) for name in os.listdir(CSRC)}
    users = {name: n for name, n in users.items() if n and name != "gp_contract.h"}
    assert users == {"gp_joint.h": 2, "gp_sparse.h": 1}, users


def test_gfx950_only_no_compat_layers():
    for name in os.listdir(CSRC):
        code = _code(os.path.join(CSRC, name))
        for token in ("__HIP_PLATFORM_AMD__", "__CUDACC__", "cuda_runtime", "cudaMalloc", "hipify", "__HIP_PLATFORM_NVIDIA__"):
            assert token not in code, (name, token)
