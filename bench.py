#!/usr/bin/env python3
"""bench.py -- BLS12-381 G1 MSM throughput on MI355X (BASELINE.json metric, configs[1]).

One "step" = one 2^20-pair G1 MSM per GPU through libgemini_hip.so (gm_g1_msm_d_partial), scalars and
bases already resident in HBM, followed -- for N > 1 -- by the all-gather of the 144-byte partial
points over RCCL and the local EC add, so that every rank ends the step holding the final group
element.  Weak scaling: every rank owns its own 2^20 pairs of one N*2^20-pair MSM.

A plain run (`bench.py --gpus 1 --steps K --warmup W`) sets up, warms up, times the K steps and prints ONE
JSON line (rank 0) with the contract fields only (metric, value, unit, higher_is_better, dtype, ms_per_step,
the configuration).  Its timed steps are the bare MSMs; with `--full` the same steps also record HIP events
around k_acc0 (the roofline's kernel time), which costs a few percent -- so do not compare a plain `value` or
`ms_per_step` with a `--full` one.  `--full` adds everything else, as one line as well:
  roofline     : the dominant kernel (k_acc0, bucket accumulate) -- algorithmic bytes per launch
                 (128 B per pair x pairs per launch) / its mean duration measured with HIP events on
                 the library's stream, against the 8 TB/s HBM peak; stage_ms of every kernel;
  cpu_baseline : the CPU restatement of the reference algorithm (oracle/, kind "port") timed on this
                 box's host cores on one full 2^20 MSM of the same inputs (rank 0, N = 1 only);
  and the further legs (fixed-base tables, batch_commit, PCIe, time_prover, psnark, strong scaling),
  which the --no-* / --*-logn options below select.
`--dump-outputs DIR` writes what the last timed step computed (rank 0): DIR/msm_result.npy, the MSM's G1
point as canonical affine coordinates, float64 of shape (2, 12) -- x and y in 32-bit little-endian limbs
(exact in float64); the point at infinity is all zeros.  The inputs are seeded: the same arguments give
the same inputs, and so the same file, from run to run.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

LOG_N = 20
R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
MADD_ISSUE_BOUND = round(1024 * 64 * 2.4e9 / (3517 * 4.5 + 876 * 2.35))  # mixed additions / s, see the roofline note
HBM_PEAK = 8.0e12  # B/s, /opt/skills/guides/MI355X_MICROARCH.md
BYTES_PER_PAIR = 128  # 32 B scalar + 96 B affine base


def host_cpus() -> dict:
    """CPUs this process may really use: logical count, affinity mask, cgroup quota (`cpu.max` = "1600000 100000" on a 256-thread
    host means 16) -- the CPU baselines run on THESE, and host threads beyond the quota get the whole process throttled"""
    logical = os.cpu_count() or 1
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = logical
    quota = None
    try:
        a, b = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if a != "max" and float(b) > 0:
            quota = float(a) / float(b)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0 and per > 0:
                quota = q / per
        except (OSError, ValueError):
            quota = None
    eff = min(logical, aff, int(quota + 0.5) if quota else logical)
    return {"logical": logical, "affinity": aff, "cgroup_quota": quota, "effective": max(eff, 1)}


def cpu_throttled_usec() -> int:
    """cumulative time the cgroup of this process has been throttled by its CPU quota (0 when unknown)"""
    for path in ("/sys/fs/cgroup/cpu.stat", "/sys/fs/cgroup/cpu/cpu.stat"):
        try:
            for line in open(path):
                k, v = line.split()[:2]
                if k == "throttled_usec":
                    return int(v)
                if k == "throttled_time":  # cgroup v1: nanoseconds
                    return int(v) // 1000
        except (OSError, ValueError):
            continue
    return 0


def uniform_fr(rng: np.random.Generator, n: int) -> np.ndarray:
    """n uniform canonical Fr scalars (255-bit draws, rejection above r), shape (n, 4) uint64."""
    r_l = np.array([(R_MOD >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
    out = np.empty((n, 4), dtype=np.uint64)
    todo = np.arange(n)
    while len(todo):
        v = rng.integers(0, 2**64, size=(len(todo), 4), dtype=np.uint64)
        v[:, 3] &= np.uint64(2**63 - 1)
        # lexicographic compare against r from the top limb
        lt = np.zeros(len(todo), dtype=bool)
        eq = np.ones(len(todo), dtype=bool)
        for k in (3, 2, 1, 0):
            lt |= eq & (v[:, k] < r_l[k])
            eq &= v[:, k] == r_l[k]
        out[todo[lt]] = v[lt]
        todo = todo[~lt]
    return out


def g1_affine_limbs(jac: np.ndarray) -> np.ndarray:
    """a Jacobian G1 point (18 u64: X, Y, Z in Montgomery form, as the library returns it) as canonical affine x, y in 32-bit
    little-endian limbs, float64 (2, 12) -- exact; the point at infinity is all zeros"""
    q = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
    r_inv = pow(1 << 384, -1, q)
    X, Y, Z = (sum(int(v) << (64 * i) for i, v in enumerate(c)) * r_inv % q for c in np.asarray(jac, dtype=np.uint64).reshape(3, 6))
    out = np.zeros((2, 12), dtype=np.float64)
    if Z:
        zi = pow(Z, -1, q)
        for row, v in enumerate((X * zi * zi % q, Y * zi * zi * zi % q)):
            out[row] = [(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)]
    return out


def snark_time_prover(gm, logn: int, with_tables: bool = True, world: int = 1, rank: int = 0, cpu_logn: int = 0, cpu_top: bool = True) -> dict:
    """second half of BASELINE.json's metric: wall time of the `Proof::new_time` span
    (src/snark/time_prover.rs:23,109) on dummy_r1cs(2^logn) with an SRS of 2^(logn+1)+1 powers
    (examples/snark.rs:69-79).  Instance and SRS are built before the timer, as in the reference.
    N > 1: the KZG key is sharded element-cyclically over the ranks (gm_ck_*, gemini_amd/csrc/sharded.cpp), every commitment is a
    local MSM + one 144-byte all-gather; the span is the max over ranks."""
    import ctypes as C
    import statistics

    from gemini_amd.circuit import dummy_r1cs
    from gemini_amd.kzg import CommitterKey
    from gemini_amd.snark import Proof

    lib = gm.capi.load()
    SPAN = "ark_gemini::snark::time_prover"
    n = 1 << logn
    rng = np.random.default_rng(2022420)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % R_MOD
    t0 = time.perf_counter()
    e = rnd()
    r1cs = dummy_r1cs(e, n)
    t_inst = time.perf_counter() - t0
    t0 = time.perf_counter()
    tau_i = rnd()
    tau = np.array([(tau_i >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
    block_sharded = world > 1 and world & (world - 1) == 0 and n // world >= 1 << 12 and os.environ.get("GM_BENCH_SHARDING", "block") == "block"
    if block_sharded:
        # N ranks, a power of two: every vector of the prover and the key in blocks, the whole prover compiled into the library
        # (gm_snark_new_time_sharded over the library's own all-gather, gemini_amd/csrc/{sharded,dist}.cpp) -- the field arithmetic
        # is sharded as well as the MSMs
        from gemini_amd.sharded import R1csShard, ShardKey, new_time_sharded

        r1cs.free()
        r1cs = R1csShard.dummy(e, n)
        ck = ShardKey(n, 10, tau)
    elif world > 1:
        # any other rank count: the native single-GPU prover over an element-cyclic share of the key (MSMs sharded, gm_ck_*)
        from gemini_amd.sharded import cyclic_committer_key

        ck = cyclic_committer_key(2 * n, 5, tau, with_g2=False)
    else:
        ck = CommitterKey.new(2 * n, 5, tau)
    t_srs = time.perf_counter() - t0

    def timed_runs(k):
        from gemini_amd import collective

        out = []
        for _ in range(k):
            if world > 1:
                collective.allgather_host(np.zeros(1, dtype=np.uint64))  # barrier through the library's own transport
            if block_sharded:
                p = new_time_sharded(r1cs, ck)
            else:
                p = Proof.new_time(r1cs, ck, native=True)  # gm_snark_new_time, the orchestration inside the library
            sp = dict(p.spans)
            if world > 1:  # the span of the slowest rank
                allt = collective.allgather_host(np.array([sp[SPAN]], dtype=np.float64).view(np.uint64))
                sp[SPAN] = float(allt.view(np.float64).max())
            out.append((sp, p))
        return out

    timed_runs(1)  # warm-up: workspaces, pool, first-touch
    runs = timed_runs(3)
    spans_sorted = sorted((r[0] for r in runs), key=lambda sp: sp[SPAN])
    med = spans_sorted[len(spans_sorted) // 2]
    import hashlib

    digest = hashlib.sha256(runs[-1][1].serialize_compressed()).hexdigest()
    per_rank = None
    coll = None
    if world > 1:
        from gemini_amd import collective

        coll = dict(collective.stats(), transport=collective.info()[2], routes=collective.stats_routes())
        # every rank's own stage breakdown of its median run (the field arithmetic is replicated, the MSMs are sharded: the
        # spread between the ranks and the share of the commitment spans say what N GPUs bought)
        import torch.distributed as dist

        mine = sorted((dict(r[1].spans) for r in runs), key=lambda sp: sp[SPAN])[len(runs) // 2]
        per_rank = [None] * world
        dist.all_gather_object(per_rank, {k: round(v, 4) for k, v in mine.items()})

    # roofline of the sumcheck kernel (k_sc_round, fused fold + next message): 192 * N algorithmic bytes per
    # sumcheck, two sumchecks per proof, against the sum of its launch durations (HIP events
    # on the library stream; this extra run has the stage timers on, which serialises the batched commitments, so
    # its wall time is not used)
    sc = None
    if world == 1:
        gm.capi.check(lib.gm_prof_enable(C.c_int(1)))
        Proof.new_time(r1cs, ck, native=True)  # the driver the timed runs use (gm_snark_new_time): the same launches, the same count
        ms = (C.c_double * 7)()
        cnt = (C.c_uint64 * 7)()
        gm.capi.check(lib.gm_prof_read(ms, cnt, C.c_int(7)))
        gm.capi.check(lib.gm_prof_enable(C.c_int(0)))
        if cnt[6]:
            bytes_sc = 2 * 192 * n
            sc = {"bound": "hbm", "kernel": "k_sc_round (fold + next message, one launch per round)", "launches": int(cnt[6]),
                  "kernel_ms_total": round(ms[6], 4), "algorithmic_bytes": bytes_sc, "achieved": round(bytes_sc / (ms[6] * 1e-3) / 1e9, 2),
                  "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": round(bytes_sc / (ms[6] * 1e-3) / HBM_PEAK, 4),
                  # products: 3 N in the first round (no fold), 2.5 per input element of every folding round (N + N/2 + ...): 8 N
                  "fr_mul_per_s": round(2 * 8 * n / (ms[6] * 1e-3)),
                  # 129 v_mad_u64_u32 + 128 v_addc_co_u32 + 8 v_mul_lo_u32 at 4.3 cycles + ~40 plain instructions per product
                  "fr_mul_issue_bound": 1.25e11,
                  "alu_frac": round(2 * 8 * n / (ms[6] * 1e-3) / 1.25e11, 4),
                  "driver": "gm_snark_new_time (the prover the metric times), stage timers on",
                  "note": "two sumchecks of length N = 2^logn; 8 N Fr products per sumcheck = 1 per 24 bytes: with a 1260-cycle product the kernel "
                          "is integer-ALU bound at <= 3 TB/s (37 % of the HBM peak) in the large rounds and launch-latency bound in the last ~15; "
                          "since round 5 the three inner products of a message accumulate unreduced (80 instead of 137 multiply-adds each, "
                          "one reduction per thread): alu_frac still counts them as whole products"}

    # The key was registered with the library's default: fixed-base window tables when they fit (gm_set_auto_tables), so the
    # runs above ARE the default configuration.  The same prover on the plain path (no tables) beside it.
    tab_c, tab_bytes = ck.bases.table_info() if block_sharded else ck.powers_of_g.table_info()
    tables = {"window_bits": tab_c, "table_bytes": tab_bytes, "built_at": "key registration (CommitterKey::new, outside the prover span)"}
    plain = None
    if world == 1 and tab_c:
        lib.gm_set_msm_table_min(C.c_size_t(1 << 62))
        pruns = timed_runs(3)
        lib.gm_set_msm_table_min(C.c_size_t(1 << 17))
        pv = sorted(r[0][SPAN] for r in pruns)
        same = hashlib.sha256(pruns[-1][1].serialize_compressed()).hexdigest() == digest
        plain = {"value": round(pv[1], 4), "unit": "s", "runs_s": [round(v, 4) for v in pv], "same_proof_bytes": same}
    r1cs.free()
    if block_sharded:
        ck.free()
    else:
        ck.powers_of_g.free()

    # CPU baseline of the SAME span: the C restatement of the reference's algorithm end to end (oracle/snark_c.py:
    # MSMs one OpenMP task per window like ark-ec, field passes and sumchecks single-threaded like the reference),
    # on a bounded instance; the device proves that instance too and the proofs must be byte-identical
    cpu = None
    if cpu_logn and world == 1:
        from oracle import snark_c, wire_ref

        # measured at TWO sizes (cpu_logn and cpu_logn + 2, 2^20 and 2^22 by default: ~5 s + ~20 s of CPU) so that the figure for
        # the size the metric is quoted on rests on a MEASURED growth ratio, not on an assumed one
        measured = {}
        # ... and, by default, AT the size the metric is quoted on (--cpu-snark-top, ~1 minute of CPU at 2^24)
        for lg in sorted({cpu_logn, cpu_logn + 2} | ({logn} if cpu_top else set())):
            if lg > logn:
                continue
            m = 1 << lg
            ck2 = CommitterKey.new(2 * m, 5, tau)
            r2 = dummy_r1cs(e, m)
            Proof.new_time(r2, ck2, native=True)
            g_runs = []
            for _ in range(3):
                p2 = Proof.new_time(r2, ck2, native=True)
                g_runs.append(p2.spans[SPAN])
            host_powers = ck2.powers_of_g.download(0, m + 1)
            # timed on the build of the restatement for today's CPUs (oracle/Makefile: x86-64-v3 + ADX, the Fq product in mulx /
            # adcx / adox asm -- what ark-ff's `asm` feature gives the reference, Cargo.toml:77-82); the portable checker build
            # beside it at the smallest size
            from oracle import oracle as orc_t

            t0 = time.perf_counter()
            with orc_t.native():
                build = orc_t._which
                port = snark_c.new_time_dummy(e, m, host_powers)
            cpu_s = time.perf_counter() - t0
            same = wire_ref.snark_proof(port, True) == p2.serialize_compressed()
            measured[lg] = {"cpu_s": round(port["spans"][SPAN], 3), "cpu_run_incl_setup_s": round(cpu_s, 1), "gpu_same_instance_s": round(sorted(g_runs)[1], 4),
                            "matches_gpu_proof_bytes": bool(same), "build": build, "spans_s": {k: round(v, 3) for k, v in port["spans"].items()}}
            if lg == cpu_logn and build == "native":
                t0 = time.perf_counter()
                slow = snark_c.new_time_dummy(e, m, host_powers)
                cpu_s += time.perf_counter() - t0
                measured[lg]["cpu_run_incl_setup_s"] = round(cpu_s, 1)
                measured[lg]["portable_build_cpu_s"] = round(slow["spans"][SPAN], 3)
                measured[lg]["portable_build_same_bytes"] = bool(wire_ref.snark_proof(slow, True) == p2.serialize_compressed())
            r2.free()
            ck2.powers_of_g.free()
            del host_powers
        lgs = sorted(measured)
        top = lgs[-1]
        ratio = (measured[top]["cpu_s"] / measured[lgs[0]]["cpu_s"]) ** (2.0 / (top - lgs[0])) if len(lgs) > 1 else None  # per factor 4 in n
        steps = (logn - top) / 2.0
        cpu = {"value": measured[top]["cpu_s"], "unit": "s", "logn": top, "cores": host_cpus()["effective"],
               "threads_busy": "<= 17 in the MSMs (one task per window, c = 15 at 2^20), 1 elsewhere", "kind": "port",
               "build": "oracle/libgemini_oracle_native.so (-march=x86-64-v3 -madx, Fq product in mulx/adcx/adox asm); the portable x86-64-v2 "
                        "checker build beside it at the smallest size (portable_build_cpu_s)",
               "sample": f"Proof::new_time on dummy_r1cs(2^k), k = {lgs}, one run each "
                         f"({sum(v['cpu_run_incl_setup_s'] for v in measured.values()):.0f} s of CPU incl. setup)",
               "measured": {str(k): v for k, v in measured.items()},
               "growth_per_4x_n_measured": round(ratio, 3) if ratio else None,
               f"at_logn_{logn}_from_measured_growth_s": round(measured[top]["cpu_s"] * (ratio ** steps), 1) if ratio else None,
               "matches_gpu_proof_bytes": all(v["matches_gpu_proof_bytes"] for v in measured.values())}
    # checker leg (like the CPU baseline: outside the timed region, oracle/ as the checker only): the proof that was
    # just timed goes through the restated VERIFIER of the reference (src/snark/verifier.rs:19-119 -- sumcheck
    # subclaims, tensor relation, pairing check against the key built from the trapdoor)
    verdict = None
    if cpu_logn and world == 1:
        from oracle import oracle as orc
        from oracle import verifier_ref as V

        p = runs[-1][1]
        I = gm.fr.fr_to_int
        J = lambda pt: orc.affine_to_ints(orc.g1_to_affine(np.asarray(pt, dtype=np.uint64)))
        msgs = lambda m: ([(I(a), I(b)) for a, b in m[0]], (I(m[1][0][0]), I(m[1][0][1])))
        tc = p.tensorcheck_proof
        ints = {"witness_commitment": J(p.witness_commitment), "zc_alpha": I(p.zc_alpha), "first_sumcheck_msgs": msgs(p.first_sumcheck_msgs),
                "second_sumcheck_msgs": msgs(p.second_sumcheck_msgs),
                "tensorcheck_proof": {"folded_polynomials_commitments": [J(c) for c in tc.folded_polynomials_commitments],
                                      "folded_polynomials_evaluations": [[I(x) for x in e2] for e2 in tc.folded_polynomials_evaluations],
                                      "evaluation_proof": J(tc.evaluation_proof),
                                      "base_polynomials_evaluations": [[I(x) for x in e3] for e3 in tc.base_polynomials_evaluations]}}
        t0 = time.perf_counter()
        try:
            V.snark_verify(ints, {"a": range(n), "x": [e]}, V.VerifierKey.from_trapdoor(tau_i, 5), m_of=V.dummy_matrix_evaluations(e, n))
            accepted = True
        except V.VerificationError:
            accepted = False
        verdict = {"accepted": accepted, "seconds": round(time.perf_counter() - t0, 2),
                   "what": "oracle/verifier_ref.py (restatement of src/snark/verifier.rs + pairing check, CPU) on the timed proof"}
    return {
        "metric": "snark time_prover",
        "unit": "s",
        "logn": logn,
        "n_gpus": world,
        "value": round(med[SPAN], 4),
        "runs_s": [round(sp[SPAN], 4) for sp in spans_sorted],
        "higher_is_better": False,
        "spans_s": {k: round(v, 4) for k, v in med.items()},
        "per_rank_spans_s": per_rank,
        "setup_s": {"dummy_r1cs_to_hbm": round(t_inst, 3), "srs_generation_on_device": round(t_srs, 3)},
        "sumcheck_roofline": sc,
        "fixed_base_tables": tables,
        "without_tables": plain,
        "cpu_baseline": cpu,
        "verifier": verdict,
        "proof_sha256": digest,
        "driver": "gm_snark_new_time (prover orchestration compiled into the library, gemini_amd/csrc/snark.cpp)" if world == 1
                  else ("gm_snark_new_time_sharded (gemini_amd/csrc/sharded.cpp): field arithmetic and key block-sharded over the ranks, "
                        "all-gathers inside the library" if block_sharded
                        else "gm_snark_new_time over an element-cyclic share of the key (gm_ck_*: MSMs sharded, field arithmetic replicated)"),
        "collectives": coll,
        "note": "median of 3 after one warm-up; instance (diagonal CSR) and SRS resident in HBM before the timer; proof elements equal the CPU "
                "restatement at logn 3/6/9 (tests/test_gpu_snark.py)",
    }


def psnark_time_prover(gm, logn: int, world: int = 1, rank: int = 0) -> dict:
    """BASELINE configs[4] (`examples/psnark --time-prover`, src/psnark/time_prover.rs:69-384) as a STRONG-scaling point: dummy_r1cs(2^logn) whole,
    one GPU through gm_psnark_new_time, N GPUs through gm_psnark_new_time_sharded -- every vector of the prover and the key in blocks over the
    ranks (gemini_amd/csrc/psnark_sharded.cpp), all-gathers inside the library.  Key of num_constraints + num_variables + 1 powers
    (examples/psnark.rs:76).  Instance, index and SRS are built before the timer, as in the reference."""
    import hashlib
    import warnings

    from gemini_amd import collective
    from gemini_amd.circuit import dummy_r1cs

    warnings.filterwarnings("ignore", message="commit: polynomial of", category=RuntimeWarning)  # the reference's key is one power short, knowingly
    SPAN = "ark_gemini::psnark::time_prover"
    n = 1 << logn
    rng = np.random.default_rng(2022420)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % R_MOD  # noqa: E731
    t0 = time.perf_counter()
    e_inst = rnd()
    r1cs = dummy_r1cs(e_inst, n)
    tau_i = rnd()
    tau = np.array([(tau_i >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
    shard = None
    if world > 1:
        from gemini_amd.sharded import PsnarkShard, PsnarkShardKey, psnark_new_time_sharded

        r1cs.free()
        r1cs = None
        shard = PsnarkShard.dummy(e_inst, n, tail_log=10)  # this rank's blocks in closed form: nothing of size n on the host
        ck = PsnarkShardKey(2 * n, shard.block, 10, tau)
        index = shard.index(ck)
        prove = lambda: psnark_new_time_sharded(shard, ck, index)  # noqa: E731
    else:
        from gemini_amd.kzg import CommitterKey
        from gemini_amd.psnark import Proof

        ck = CommitterKey.new(2 * n, 5, tau)
        index = Proof.index(ck, r1cs)
        prove = lambda: Proof.new_time(ck, r1cs, index, native=True)  # noqa: E731
    t_setup = time.perf_counter() - t0
    gm.capi.mem_reset_peak()
    spans, proof = [], None
    for i in range(4):  # one warm-up + 3
        if world > 1:
            collective.allgather_host(np.zeros(1, dtype=np.uint64))
        proof = prove()
        t = proof.spans[SPAN]
        if world > 1:
            t = float(collective.allgather_host(np.array([t], dtype=np.float64).view(np.uint64)).view(np.float64).max())  # the slowest rank
        if i:
            spans.append((t, dict(proof.spans)))
    spans.sort(key=lambda x: x[0])
    digest = hashlib.sha256(proof.serialize_compressed()).hexdigest()
    mem = gm.capi.mem_stats()
    out = {
        "metric": "psnark time_prover", "unit": "s", "logn": logn, "n_gpus": world, "scaling": "strong", "value": round(spans[1][0], 4),
        "runs_s": [round(t, 4) for t, _ in spans], "higher_is_better": False, "spans_s": {k: round(v, 4) for k, v in spans[1][1].items()},
        "setup_s": round(t_setup, 2), "proof_sha256": digest, "peak_in_use_GB_rank0": round(mem["in_use_peak"] / 1e9, 2),
        "driver": "gm_psnark_new_time (gemini_amd/csrc/psnark.cpp)" if world == 1 else
                  f"gm_psnark_new_time_sharded (gemini_amd/csrc/psnark_sharded.cpp): blocks of {shard.block} elements over {world} ranks, the same proof bytes as one GPU "
                  "(tests/test_gpu_dist_native.py)",
    }
    if world > 1:
        out["collectives"] = dict(collective.stats(), routes=collective.stats_routes())
        shard.free()
        ck.free()
    if r1cs is not None:
        r1cs.free()
    return out


def main():
    # the CPU baselines' OpenMP workers sleep when idle instead of spinning: the container's CPU quota (16 of 256 hardware threads on
    # the pool's boxes) is shared with the host side of the device path that is timed next
    os.environ.setdefault("OMP_WAIT_POLICY", "PASSIVE")
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: 0.4 s of timed steps behind 75 ms of warm-up -- one 75 ms window of 20 steps was seen to catch a clock
    # ramp after an idle period (238 instead of 278 Mscalar/s once in ~30 runs)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--logn", type=int, default=LOG_N, help="pairs per GPU per step = 2^logn (default: BASELINE configs[1])")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed to DIR/msm_result.npy (rank 0; see the module docstring)")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline: roofline and stage_ms, the CPU baselines and the further legs "
                    "(the options below act only with --full)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--headline-only", action="store_true", help="with --full: the timed headline loop and its roofline / stage_ms only (what the rocprofv3 "
                    "summary under profiles/ is taken from: the extra legs overlap kernels on several streams, which stretches their durations)")
    ap.add_argument("--no-tables", action="store_true", help="skip the extra fixed-base-table measurement")
    ap.add_argument("--cpu-snark-logn", type=int, default=20, help="instance size of the time_prover CPU baseline (0 = skip)")
    ap.add_argument("--no-cpu-snark-top", action="store_true", help="do not run the time_prover CPU baseline at --snark-logn itself (about a minute at 2^24), "
                    "only at --cpu-snark-logn and two powers above it")
    # sizes of the strong-scaling legs: large enough that one rank's share on 8 GPUs is still throughput-bound (a share of psnark -i 22 is 45 % accumulation,
    # of -i 24 most of it: profiles/r6_exposed_time.md; an MSM of 2^23 pairs runs at 1.5 x the rate of one of 2^21)
    ap.add_argument("--psnark-logn", type=int, default=24, help="also time psnark::Proof::new_time on dummy_r1cs(2^k): one GPU natively, N GPUs block-sharded (0 = skip)")
    ap.add_argument("--strong-msm-logn", type=int, default=26, help="also time ONE MSM of 2^k pairs in total, split n / g over the ranks (strong scaling; 0 = skip)")
    ap.add_argument("--snark-logn", type=int, default=24, help="also time snark::Proof::new_time on dummy_r1cs(2^k) (N=1 only; 0 = skip)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:
        args.headline_only = True  # the plain run: the headline loop alone, without even its roofline pass (below)
    if args.headline_only:
        args.no_cpu_baseline = True
        args.no_tables = True
        args.snark_logn = 0
        args.psnark_logn = 0
        args.strong_msm_logn = 0

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with {args.gpus} ranks (WORLD_SIZE={world})")
    # test hooks (not used by the driver): GM_BENCH_BACKEND=gloo + GM_BENCH_SINGLE_DEVICE=1 run the
    # N > 1 code path with every rank on GPU 0 of a one-GPU box (collectives on CPU tensors)
    backend = os.environ.get("GM_BENCH_BACKEND", "nccl")
    if os.environ.get("GM_BENCH_SINGLE_DEVICE") == "1":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    coll_dev = "cuda" if backend == "nccl" else "cpu"

    import gemini_amd as gm
    from gemini_amd.msm import g1_sum

    gm.capi.init(local_rank)
    lib = gm.capi.load()
    transport_note = None
    if world > 1:
        # the all-gathers of the N > 1 path run INSIDE the library (gemini_amd/csrc/dist.cpp): its own RCCL communicator over xGMI on a
        # GPU node (the unique id travels over torch.distributed), the torch process group behind a hook with the gloo test backend.
        # GM_BENCH_TRANSPORT = rccl | hook | shm overrides; an RCCL communicator that cannot be built or fails its self-test falls back
        # to the hook and says so in the output.
        from gemini_amd import collective

        want = os.environ.get("GM_BENCH_TRANSPORT") or ("rccl" if backend == "nccl" else "hook")
        ok = 0
        if want == "rccl":
            try:
                # one node: the ranks meet in a shared-memory segment that carries the RCCL id and then STAYS OPEN as the side channel
                # of the small field payloads (64 bytes per sumcheck round, evaluations); partial G1 points take ncclAllGather
                collective.init_rccl_node(rank, world, "/gm_bench_%s" % os.environ.get("MASTER_PORT", "0"))
                collective.selftest()
                ok = 1
            except Exception as ex:  # noqa: BLE001
                transport_note = f"library RCCL communicator unavailable on rank {rank} ({ex}); fell back to the torch.distributed hook"
            flags = [None] * world
            dist.all_gather_object(flags, ok)
            if not all(flags):
                collective.finalize()
                want = "hook"
                transport_note = transport_note or "library RCCL communicator unavailable on a peer; fell back to the torch.distributed hook"
        if want == "shm":
            collective.init_shm(rank, world, "/gm_bench_%s" % os.environ.get("MASTER_PORT", "0"))
        elif want == "hook":
            collective.init_hook_torch()
        collective.selftest()
    n = 1 << args.logn
    rng = np.random.default_rng(0x47454D494E49 + rank)

    # bases: uniform G1 points k_i * G generated on device (benches/msm_bench.rs:23-26 shape);
    # the generator in arkworks Montgomery form:
    gx = 0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB
    gy = 0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1
    q = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
    mont = lambda v: [(((v << 384) % q) >> (64 * i)) & (2**64 - 1) for i in range(6)]
    g_aff = np.array(mont(gx) + mont(gy), dtype=np.uint64)
    ks = uniform_fr(rng, n)
    # scalars: two resident sets, alternated, so no step can reuse anything from the previous one.  All host-side generation
    # comes BEFORE the device-side set-up, so that the device does not sit idle (and clock down) between its set-up work and
    # the first warm-up step
    host_scalars = [uniform_fr(rng, n) for _ in range(2)]
    # the headline is the PLAIN one-call MSM: no fixed-base tables for these bases (the library builds them by default at
    # registration; the table path is reported beside it as `with_fixed_base_tables`)
    gm.capi.check(lib.gm_set_auto_tables(C.c_int(0), C.c_size_t(0)))
    bases = gm.G1Bases.fixed_base(g_aff, ks)
    dev_scalars = [torch.from_numpy(s.view(np.int64)).cuda() for s in host_scalars]
    torch.cuda.synchronize()

    def step(i: int) -> np.ndarray:
        d = dev_scalars[i & 1]
        part = bases.msm_device(d.data_ptr(), n, mont=False, partial=world > 1)
        if world == 1:
            return part
        # the final reduce of the partial G1 points: ONE all-gather of 144 bytes inside the library, EC adds on every rank
        return g1_sum(collective.allgather_host(part, collective.CLASS_G1))

    def barrier():
        if world > 1:
            collective.allgather_host(np.zeros(1, dtype=np.uint64))  # through the transport the timed steps use
        torch.cuda.synchronize()

    results = {}
    for i in range(args.warmup):
        results[i & 1] = step(i)
    # HIP events around k_acc0 ONLY in the timed steps (mode 2): an event record between two kernels of a call is a ~10 us bubble
    # on the stream, and the dominant kernel is the one the contract wants timed live; the other stages are timed in a short
    # untimed pass after the loop (--full only: a plain run times the bare steps)
    if args.full:
        gm.capi.check(lib.gm_prof_enable(C.c_int(2)))
    barrier()
    throttled0 = cpu_throttled_usec()
    t0 = time.perf_counter()
    for i in range(args.steps):
        r = step(i)
        assert (r == results.setdefault(i & 1, r)).all(), "non-deterministic MSM result"
    barrier()
    elapsed = time.perf_counter() - t0
    throttled_in_loop = cpu_throttled_usec() - throttled0
    if world > 1:
        elapsed = float(collective.allgather_host(np.array([elapsed], dtype=np.float64).view(np.uint64)).view(np.float64).max())
    if args.dump_outputs and rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "msm_result.npy"), g1_affine_limbs(r))
    def config() -> dict:
        """read when the line is printed: with --full, the routes then count the collectives of every leg, not only the headline's"""
        return {
            "workload": f"2^{args.logn} G1 MSM per GPU (BASELINE configs[1]: 2^20 G1 MSM on one MI355X)",
            "pairs_per_gpu": n,
            "parallelism": f"pairs sharded over {world} GPU(s), all-gather of 144-byte partial points + local EC add",
            "collective": None if world == 1 else {"transport": collective.info()[2], "inside_library": "gm_dist_allgather_host_class (gemini_amd/csrc/dist.cpp)",
                                                   # which route each class of collective took: partial G1 points (the per-MSM reduce) vs field values / barriers
                                                   "routes": collective.stats_routes(), "note": transport_note},
        }

    headline = {
        "metric": "BLS12-381 G1 MSM throughput",
        "value": round(world * n * args.steps / elapsed / 1e6, 3),
        "unit": "Mscalar/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u32x12 Montgomery Fq (381-bit integer), u32x8 Fr",
        "data": "synthetic: uniform random Fr scalars x uniform random G1 affine points (k_i*G), seeded",
        "config": None,  # config(), filled in when the line is printed
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(dict(headline, config=config())))
        if world > 1:
            dist.destroy_process_group()
        return

    ms = (C.c_double * 7)()
    cnt = (C.c_uint64 * 7)()
    gm.capi.check(lib.gm_prof_read(ms, cnt, C.c_int(7)))
    acc0_mhz = C.c_double(0.0)
    gm.capi.check(lib.gm_prof_read_clock(C.byref(acc0_mhz)))  # clock64() / wall_clock64() inside k_acc0, over the timed steps
    acc0_mhz = acc0_mhz.value
    acc0_live_ms, acc0_live_cnt = ms[3], cnt[3]
    gm.capi.check(lib.gm_prof_enable(C.c_int(1)))  # every stage, untimed: stage_ms of the other kernels
    for i in range(min(args.steps, 10)):
        step(i)
    barrier()
    gm.capi.check(lib.gm_prof_read(ms, cnt, C.c_int(7)))
    ms[3], cnt[3] = acc0_live_ms, acc0_live_cnt  # k_acc0: the live figure of the timed steps
    gm.capi.check(lib.gm_prof_enable(C.c_int(0)))

    # extra (not the headline): the same MSM with fixed-base window tables for the resident SRS
    tables = None
    if world == 1 and not args.no_tables:
        tp0 = time.perf_counter()
        bases.precompute(0)
        t_pre = time.perf_counter() - tp0
        for i in range(2):
            rt = step(i)
            assert (rt == results[i & 1]).all(), "table path result differs from the plain path"
        barrier()
        tt0 = time.perf_counter()
        for i in range(args.steps):
            step(i)
        barrier()
        t_tab = time.perf_counter() - tt0
        tables = {"value": round(n * args.steps / t_tab / 1e6, 3), "unit": "Mscalar/s", "ms_per_step": round(t_tab / args.steps * 1e3, 4),
                  "window_bits": 20, "table_bytes": 13 * n * 96, "precompute_s": round(t_pre, 3),
                  "note": "gm_g1_bases_precompute: 2^(20w)*P_i resident in HBM, one shared bucket set; results identical to the plain path"}
    # extra (not the headline): CommitterKey::batch_commit shape -- 8 MSMs per call through gm_g1_msm_v_batch,
    # which overlaps the host tail (bit-plane Horner) of MSM j with the kernels of MSM j+1
    batch = None
    if world == 1 and not args.headline_only:
        from gemini_amd.fr import FrVec

        lib.gm_set_msm_table_min(C.c_size_t(1 << 62))  # plain path even if tables were just built
        vecs = [FrVec.from_host(s) for s in host_scalars]  # the same limbs read as Montgomery residues
        seq = [bases.msm_vec(v) for v in vecs]
        kb = 8
        got = bases.msm_vec_batch([vecs[j & 1] for j in range(kb)], [n] * kb)
        assert all((got[j] == seq[j & 1]).all() for j in range(kb)), "batched MSM differs from the one-call MSM"
        reps = max(1, args.steps // kb)
        barrier()
        tb0 = time.perf_counter()
        for _ in range(reps):
            bases.msm_vec_batch([vecs[j & 1] for j in range(kb)], [n] * kb)
        barrier()
        t_b = time.perf_counter() - tb0
        batch = {"value": round(n * kb * reps / t_b / 1e6, 3), "unit": "Mscalar/s", "ms_per_msm": round(t_b / (kb * reps) * 1e3, 4),
                 "msms_per_call": kb, "calls": reps, "note": "gm_g1_msm_v_batch, no fixed-base tables; results identical to one-call MSMs"}
        for v in vecs:
            v.free()
        lib.gm_set_msm_table_min(C.c_size_t(1 << 17))
    # extra (never `value`): the same MSM when the boundary hands over HOST buffers -- scalars only (SRS resident,
    # gm_g1_msm_h: 32 MiB over PCIe per call) and the one-shot gm_g1_msm (bases 96 MiB + scalars 32 MiB per call)
    pcie = None
    if world == 1 and not args.headline_only:
        from gemini_amd.msm import VariableBaseMSM

        hb_full = bases.download()
        r_h = bases.msm_bigint(host_scalars[0])
        assert (r_h == results[0]).all()
        barrier()
        tp0 = time.perf_counter()
        for i in range(5):
            bases.msm_bigint(host_scalars[i & 1])
        barrier()
        t_h = (time.perf_counter() - tp0) / 5
        r_o = VariableBaseMSM.msm_bigint(hb_full, host_scalars[0])
        assert (r_o == results[0]).all()
        barrier()
        tp0 = time.perf_counter()
        for i in range(3):
            VariableBaseMSM.msm_bigint(hb_full, host_scalars[i & 1])
        barrier()
        t_o = (time.perf_counter() - tp0) / 3
        pcie = {"scalars_from_host_Mscalar_per_s": round(n / t_h / 1e6, 2), "scalars_from_host_ms": round(t_h * 1e3, 3),
                "bases_and_scalars_from_host_Mscalar_per_s": round(n / t_o / 1e6, 2), "bases_and_scalars_from_host_ms": round(t_o * 1e3, 3),
                "note": "pageable numpy buffers; PCIe-inclusive, reported for DESIGN.md only"}
        del hb_full
        # a stream larger than one call: 2^23 pairs resident in page-locked HOST memory through two 2^20-pair device
        # slots (gm_g1_msm_stream_*: copy of chunk i + 1 under the kernels of chunk i) -- the bounded-memory form
        from gemini_amd.msm import HostMsmStream, pinned_empty

        ns = 1 << 23
        big = gm.G1Bases.fixed_base(g_aff, uniform_fr(rng, ns))
        pb, ps = pinned_empty((ns, 12)), pinned_empty((ns, 4))
        pb[:] = big.download()
        ps[:] = uniform_fr(rng, ns)
        d_big = torch.from_numpy(np.asarray(ps).view(np.int64)).cuda()
        torch.cuda.synchronize()
        r_res = big.msm_device(d_big.data_ptr(), ns, mont=False)
        st = HostMsmStream(1 << 20)
        t_s = 1e9
        for _ in range(2):
            barrier()
            tp0 = time.perf_counter()
            st.add(pb, ps)
            r_s = st.finalize()
            t_s = min(t_s, time.perf_counter() - tp0)
        st.free()
        assert (r_s == r_res).all(), "streamed MSM differs from the resident one"
        pcie["streamed_2p23_pairs_from_pinned_host_Mscalar_per_s"] = round(ns / t_s / 1e6, 2)
        pcie["streamed_ms"] = round(t_s * 1e3, 2)
        pcie["streamed_note"] = "bases AND scalars host-resident (1 GiB), 2 device slots of 2^20 pairs, same result as the resident one-call MSM"
        big.free()
        del pb, ps, d_big
    stage_names = ["digits_hist", "scan", "scatter", "acc0", "merge", "reduce", "sc_round"]
    # per STEP (= one one-call MSM: `launches_per_step` in the output says how many launches of each stage that is)
    steps_of = lambda i: args.steps if i == 3 else min(args.steps, 10)  # noqa: E731 -- k_acc0 live in the timed steps, the rest in the pass after
    stages = {k: (ms[i] / steps_of(i) if cnt[i] else None) for i, k in enumerate(stage_names)}
    launches = {k: (cnt[i] / steps_of(i) if cnt[i] else None) for i, k in enumerate(stage_names)}

    # HBM traffic of the dominant kernel: NOT measured in this run -- hardware counters need rocprofv3 --pmc passes
    # of their own (tools/profile_round.sh); the figure of the committed passes of this library is quoted with its
    # source (profiles/r5_pmc_msm20.json says how it was collected and corrected)
    traffic, traffic_source = None, None
    for tag in ("r6", "r5", "r4", "r3", "r2", "r1"):
        try:
            with open(os.path.join(ROOT, "profiles", f"{tag}_pmc_msm20.json")) as fh:
                if args.logn == LOG_N:
                    traffic = json.load(fh)["kernels"]["gm::k_acc0"]["hbm_bytes_corrected"]
                    traffic_source = f"profiles/{tag}_pmc_msm20.json (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of `bench.py --headline-only`; not re-measured in this run)"
                    break
        except (OSError, KeyError, ValueError):
            continue

    # second metric (every rank takes part when N > 1: the key is sharded)
    tp = None
    hb_for_cpu = bases.download() if (world == 1 and not args.no_cpu_baseline) else None
    if args.snark_logn > 0:
        bases.free()  # the prover's key (2^25 + 1 points) and its vectors want the memory
        gm.capi.check(lib.gm_set_auto_tables(C.c_int(0 if args.no_tables else 1), C.c_size_t(0)))  # the library default
        try:
            tp = snark_time_prover(gm, args.snark_logn, with_tables=not args.no_tables, world=world, rank=rank,
                                   cpu_logn=0 if args.no_cpu_baseline else args.cpu_snark_logn, cpu_top=not args.no_cpu_snark_top)
        except Exception as exc:  # noqa: BLE001 -- N > 1 has only ever run with gloo on one shared GPU (no multi-GPU node was available
            # to the builder): a failure of the second metric there must not take the headline line with it.  On one GPU it is a bug.
            if world == 1:
                raise
            import traceback

            tp = {"metric": "snark time_prover", "error": repr(exc), "traceback": traceback.format_exc()[-1500:]}
    second_metric_errors = {}
    if isinstance(tp, dict) and "error" in tp:
        second_metric_errors["time_prover"] = tp["error"]

    def guarded(name, fn):
        """a further metric of the N > 1 run must not take the headline with it -- but its failure is printed loudly and lands at the TOP level
        of the JSON line ("second_metric_error"), not inside a nested record the driver would read as rc 0"""
        try:
            return fn()
        except Exception as exc:  # noqa: BLE001 -- also on one GPU: the headline line (the contract) must not be lost to a later leg
            import traceback

            sys.stderr.write(f"[bench rank {rank}] {name} FAILED: {exc!r}\n{traceback.format_exc()}\n")
            second_metric_errors[name] = repr(exc)
            return {"metric": name, "error": repr(exc), "traceback": traceback.format_exc()[-1500:]}

    # STRONG scaling of the MSM (benches/msm_bench.rs:17-51 shape at a fixed size): ONE MSM of 2^k pairs in total, ceil(2^k / g) per rank, the
    # partial points all-gathered (144 B) and added on every rank.  The weak-scaling headline above cannot say what N GPUs buy for one MSM
    strong = None
    if args.strong_msm_logn > 0:
        def strong_msm():
            total = 1 << args.strong_msm_logn
            per = -(-total // world)
            mine = max(min(per, total - rank * per), 0)
            rng_s = np.random.default_rng(0x5354524F4E47 + rank)
            sb = gm.G1Bases.fixed_base(g_aff, uniform_fr(rng_s, max(mine, 1)))
            dsc = torch.from_numpy(uniform_fr(rng_s, max(mine, 1)).view(np.int64)).cuda()
            torch.cuda.synchronize()

            def one():
                part = sb.msm_device(dsc.data_ptr(), mine, mont=False, partial=world > 1)
                return part if world == 1 else g1_sum(collective.allgather_host(part, collective.CLASS_G1))

            ref = one()
            one()
            barrier()
            t1 = time.perf_counter()
            k = 5
            for _ in range(k):
                r2 = one()
                assert (r2 == ref).all(), "non-deterministic MSM result"
            barrier()
            dt = (time.perf_counter() - t1) / k
            if world > 1:
                dt = float(collective.allgather_host(np.array([dt], dtype=np.float64).view(np.uint64)).view(np.float64).max())
            sb.free()
            return {"metric": "G1 MSM, fixed total size", "scaling": "strong", "pairs_total": total, "pairs_per_gpu": per, "n_gpus": world, "ms_per_msm": round(dt * 1e3, 4),
                    "Mscalar_per_s": round(total / dt / 1e6, 2), "note": "plain one-call MSM per rank (no tables), all-gather of 144-byte partial points inside the library"}

        strong = guarded("strong_scaling_msm", strong_msm)
    ptp = None
    if args.psnark_logn > 0:
        ptp = guarded("psnark_time_prover", lambda: psnark_time_prover(gm, args.psnark_logn, world=world, rank=rank))
    if rank == 0:
        acc0_ms = stages["acc0"]
        achieved = BYTES_PER_PAIR * n / (acc0_ms * 1e-3) / 1e9 if acc0_ms else None
        out = {
            **headline,
            "config": config(),  # after every leg, as the routes say
            "roofline": {
                "bound": "hbm",
                "kernel": "k_acc0 (bucket accumulate)",
                "achieved": round(achieved, 3) if achieved else None,
                "peak": HBM_PEAK / 1e9,
                "unit": "GB/s",
                "frac": round(achieved * 1e9 / HBM_PEAK, 6) if achieved else None,
                "traffic": traffic,
                "traffic_source": traffic_source,
                # k_acc0 is launched `launches_per_step` times per step (one per window group, back to back on one
                # stream); kernel_ms is their SUM, i.e. the time the kernel needs for the bytes of one whole MSM
                "kernel_ms": round(acc0_ms, 4) if acc0_ms else None,
                "launches_per_step": launches["acc0"],
                "kernel_ms_per_launch": round(acc0_ms / launches["acc0"], 4) if acc0_ms else None,
                "algorithmic_bytes_per_launch": BYTES_PER_PAIR * n / launches["acc0"] if acc0_ms else None,
                "algorithmic_bytes_per_step": BYTES_PER_PAIR * n,
                "note": "integer-ALU bound: one XYZZ mixed addition = one asm statement of 3055 v_mad_u64_u32 (radix 2^30, 13 limbs, 9 Montgomery "
                        "reductions; gen_madd30.py); HBM fraction reported as the contract asks",
                # the truthful utilisation figure: mixed additions per second of the kernel (16 windows x n)
                # against the instruction-issue bound of the statement -- 3517 half-rate (v_mad_u64_u32, v_mul_lo_u32,
                # v_lshrrev_b64, v_addc_co_u32, v_alignbit_b32, v_or3_b32) + 876 full-rate instructions
                # (`python3 gemini_amd/csrc/gen_madd30.py --selftest` prints the mix), 4.5 / 2.35 cycles per wave each
                # (tools/ubench_isa.hip, tools/gen_ubench_regs.py), 1024 SIMDs x 64 lanes at 2.4 GHz -> 8.79 G additions/s
                "madd_per_s": round(16 * n / (acc0_ms * 1e-3)) if acc0_ms and args.logn == LOG_N else None,
                "madd_issue_bound": MADD_ISSUE_BOUND,
                "alu_frac": round(16 * n / (acc0_ms * 1e-3) / MADD_ISSUE_BOUND, 4) if acc0_ms and args.logn == LOG_N else None,
                # the bound above is priced at the nominal 2.4 GHz; this is the clock the kernel actually ran at in the timed steps
                # (read inside k_acc0: shader cycles against the constant 100 MHz counter) and the fraction at THAT clock
                "shader_clock_mhz_in_kernel": round(acc0_mhz, 1) if acc0_mhz else None,
                "alu_frac_at_measured_clock": round(16 * n / (acc0_ms * 1e-3) / (MADD_ISSUE_BOUND * acc0_mhz / 2400.0), 4)
                if acc0_ms and acc0_mhz and args.logn == LOG_N else None,
            },
            "stage_ms": {k: (round(v, 4) if v is not None else None) for k, v in stages.items()},
            # the host side of a one-call MSM (helper threads, window Horner) runs on the CPUs the container may use; a quota
            # exhausted by pollers or by other tenants throttles the whole process for the rest of a 100 ms period
            "host": dict(host_cpus(), cpu_throttled_usec_in_timed_steps=int(throttled_in_loop)),
            # the XCD partition of a batch (one XCD for the tails of the calls, seven for the accumulations) acts in batch_commit and
            # in the provers, not in the one-call headline
            "runtime": gm.capi.runtime_info(),
        }
        if world == 1 and not args.no_cpu_baseline:
            # the CPU restatement of the reference algorithm (arkworks window rule, signed digits,
            # one task per window), timed on this box's host cores on ONE full MSM of the same inputs
            from oracle import oracle as orc

            orc.build()
            hb = hb_for_cpu
            cores = host_cpus()["effective"]
            # the TIMED leg runs the build of the restatement for today's CPUs (oracle/Makefile: x86-64-v3 + ADX, the Fq product in
            # mulx / adcx / adox asm, branch-free additions -- the reference runs ark-ff with its `asm` feature, Cargo.toml:77-82);
            # the portable x86-64-v2 checker build is timed beside it
            with orc.native():
                build = orc._which
                orc.msm_pippenger(hb[: 1 << 12], host_scalars[0][: 1 << 12], threads=0)  # thread pool up
                t1 = time.perf_counter()
                exp = orc.msm_pippenger(hb, host_scalars[0], threads=0)
                cpu_s = time.perf_counter() - t1
            t1 = time.perf_counter()
            exp_p = orc.msm_pippenger(hb, host_scalars[0], threads=0)
            cpu_p = time.perf_counter() - t1
            want = orc.affine_to_ints(orc.g1_to_affine(results[0]))
            same = orc.affine_to_ints(orc.g1_to_affine(exp)) == want and orc.affine_to_ints(orc.g1_to_affine(exp_p)) == want
            out["cpu_baseline"] = {
                "value": round(n / cpu_s / 1e6, 4),
                "unit": "Mscalar/s",
                "cores": cores,
                "threads_busy": "<= 17: one OpenMP task per window (c = 15, 17 windows at 2^20), the reference's parallel grain",
                "kind": "port",
                "build": f"{build}: -march=x86-64-v3 -madx, Fq product in mulx / adcx / adox asm" if build == "native" else "portable (host without BMI2 / ADX)",
                "portable_build_value": round(n / cpu_p / 1e6, 4),
                "sample": f"one full 2^{args.logn} MSM of the benchmark inputs ({cpu_s:.2f} s; portable x86-64-v2 build {cpu_p:.2f} s), OpenMP one task per window",
                "matches_gpu_result": bool(same),
            }
            # BASELINE configs[0]: the shape of benches/msm_bench.rs:21-32 at 2^18 pairs -- the CPU restatement timed there too, and the device
            # result on the same pairs equal to it
            m18 = min(1 << 18, n)
            with orc.native():
                t1 = time.perf_counter()
                exp18 = orc.msm_pippenger(hb[:m18], host_scalars[0][:m18], threads=0)
                cpu18 = time.perf_counter() - t1
            got18 = gm.VariableBaseMSM.msm_bigint(hb[:m18], host_scalars[0][:m18])
            t1 = time.perf_counter()
            for _ in range(5):
                gm.VariableBaseMSM.msm_bigint(hb[:m18], host_scalars[0][:m18])
            dev18 = (time.perf_counter() - t1) / 5
            out["msm_bench_shape_2p18"] = {
                "config": "BASELINE configs[0]: benches/msm_bench.rs 2^18 BLS12-381 G1 MSM (the reference's own CPU-runnable case)",
                "cpu_restatement_ms": round(cpu18 * 1e3, 2), "cpu_Mscalar_per_s": round(m18 / cpu18 / 1e6, 4), "cores": cores,
                "device_ms_host_buffers": round(dev18 * 1e3, 3), "device_note": "gm_g1_msm from HOST bases and scalars (upload included: the msm_bigint call shape)",
                "matches_gpu_result": bool(orc.affine_to_ints(orc.g1_to_affine(exp18)) == orc.affine_to_ints(orc.g1_to_affine(got18))),
            }
        if tables:
            out["with_fixed_base_tables"] = tables
        if batch:
            out["batch_commit_pipelined"] = batch
        if pcie:
            out["pcie_inclusive"] = pcie
        if tp is not None:
            out["time_prover"] = tp
        if strong is not None:
            out["strong_scaling_msm"] = strong
        if ptp is not None:
            out["psnark_time_prover"] = ptp
        if second_metric_errors:
            out["second_metric_error"] = second_metric_errors
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
