#!/usr/bin/env python3
"""Headline benchmark: secp256k1 ECDSA witness fills/sec at batch 2^16 per GPU (BASELINE.json metric).

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path (p2e_ecdsa_verify_witness_batch: all 82 615 hot-path generator
outputs of verify_secp256k1_message_circuit) over one batch of 2^16 synthetic valid signatures PER GPU,
inputs already resident in HBM, output columns written to HBM.  One process per GPU; the batch is
sharded by contiguous signature ranges with no data-path collective ("scaling": "weak": per-GPU work is
fixed as N grows).  Rank 0 prints ONE JSON line.

  --scaling strong   the metric's literal shape: ONE global batch of 2^16 split over the N ranks (8 192
                     signatures per GPU at N = 8).  value = the whole batch / the max-over-ranks time of the fill;
                     the RCCL exchange that assembles the full column matrix on every rank (north star) is reported
                     beside it in "strong": alone, and pipelined with the fill (column blocks are exchanged as the
                     kernels finish them, plonky2-ecdsa_amd/dist.py ColumnAssembly) -> "value_with_allgather".
                     --compact assembles the compact container instead (28 % fewer bytes over xGMI).
  N > 1, default (weak) mode, with --full: the line ALSO carries that "strong" object -- the same measurements on ONE
                     global batch of 2^16 after the timed weak region -- so that whichever way the driver launches N
                     ranks, the metric's literal configuration is on the line (--no-strong-leg skips it).

  --dump-outputs DIR after the timed steps, write what the last step computed as DIR/<name>.npy (float64; a u64 column
                     splits exactly into its two 32-bit halves): the columns of 32 signatures picked with a fixed seed
                     (columns_lo32 / columns_hi32, shape (columns, 32); --compact: narrow / wide_lo32 / wide_hi32), and
                     the err and valid flags of the whole batch.  At most 43 MB; rank 0 only.  Inputs are seeded, so two
                     builds can be compared output for output.

A plain run (no --full) sets up, warms up, times --steps steps and prints the line with the objects that come from those
steps: phase_ms_per_step, whole_fill, roofline, roofline_k_expand, roofline_k_expand_fb_run, median_step_ms.  The
objects below that take runs of their own (roofline_limb_split, cpu_baseline*, checked_vs_oracle, p256_verify) and the
weak mode's "strong" object are only measured with --full.

Extra objects on the line:
  roofline     the dominant kernel, k_expand_runs (the MSM double/double/conditional-add loop: 59 495 of the
               82 615 columns, one launch per schedule segment of the loop).  achieved = algorithmic bytes
               per launch / average launch duration, the duration measured live with HIP events on the
               stream the kernel runs on (p2e_last_phase_ms).  traffic = HBM bytes per launch from the
               rocprofv3 PMC summary committed under profiles/ (null if absent).
  roofline_k_expand   the same figures for k_expand (window table and the three trailing adds: 6 006 columns, one
               curve op per workgroup row).
  roofline_k_expand_fb_run   the same for k_expand_fb_run (the 66 fixed-base windows walked as one run per signature:
               16 566 columns, one launch per step).
  roofline_limb_split   the 29-bit limb-split kernel (k_split, p2e_limb_split) on 2^26 packed 256-bit values:
               104 algorithmic bytes per element (32 in + 72 out), torch events on the stream it runs on.
  cpu_baseline oracle/libp2e_oracle.so (C restatement of the reference's CPU algorithm: affine ops, one
               Fermat inversion per inverse, OpenMP over signatures) timed on a bounded sample on the
               host cores of this box.  kind "port": the Rust reference cannot be built offline.
  cpu_baseline_optimised   the same C code with Montgomery batch inversion across lock-step groups of 256
               signatures (BASELINE.md section 2 variant b): the baseline a careful CPU implementation would set.
  checked_vs_oracle   signatures of the LAST timed output buffer compared column by column with the C oracle (--full
               default: every signature of the batch, after the timed region; --check K asks for it in any run).
  p256_verify  (N = 1) the widened path on the same line: verify_p256_message_circuit (gadgets/ecdsa.rs:55-78) as a curve
               program, batch 2^16, 115 557 columns per fill: fills/s (median of 5 synchronous calls), whole-fill share of
               the HBM peak, and the expansion kernels' share from the library's HIP-event pairs.  Outside the timed
               region of the headline metric; never part of `value`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# HIP multiplexes streams onto this many hardware queues (default 4); the pipeline uses three streams per
# context and kernels that share a queue run in order.  Must be set before the HIP runtime starts.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

BYTES_PER_FILL = 661080          # 160 B packed inputs + 82 615 * 8 B outputs
HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: 8 TB/s spec (6.29 TB/s measured copy)


def usable_cores(omp_max):
    """Threads this process may really run: affinity mask and cgroup CPU quota, not the host's core count."""
    n = omp_max
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def p256_leg(p2e, torch, ctx, dev, n):
    """verify_p256_message_circuit witnesses of n synthetic P-256 signatures through the curve-program entry point."""
    import numpy as np
    b = p2e.synth_signatures_curve(p2e.CURVE_P256, seed=777, n=1)      # any multiple of G serves as the circuit's rand() point
    blind = (int.from_bytes(bytes(b[3][0]), "little"), int.from_bytes(bytes(b[4][0]), "little"))
    prog = p2e.CurveProgram(ctx, p2e.CP_VERIFY, p2e.CURVE_P256, blind)
    # host-side synthesis of P-256 signatures is two generic scalar multiplications each (no fixed-base table on the host):
    # 2 048 distinct valid signatures, tiled over the batch (the kernels' work does not depend on the values)
    distinct = min(n, 2048)
    base = p2e.synth_signatures_curve(p2e.CURVE_P256, seed=4, n=distinct)
    sig = [torch.from_numpy(np.tile(a, ((n + distinct - 1) // distinct, 1))[:n].copy()).to(dev) for a in base]
    ld = n + 16
    cols = torch.empty((prog.num_cols, ld), dtype=torch.int64, device=dev)
    err = torch.empty(n, dtype=torch.uint8, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    call = lambda: prog.verify_witness_batch(*sig, cols=cols[:, :n], err=err, valid=valid, ld=ld)[3]
    bad = call()
    torch.cuda.synchronize()
    assert bad == 0 and int(valid.sum()) == n, "synthetic P-256 signatures must all verify"
    ts, ph = [], []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
        ph.append(ctx.last_phase_ms())
    med = sorted(ts)[len(ts) // 2]
    kinds = (("expand", "kc_expand"), ("runs", "kc_expand_runs"), ("fbrun", "kc_expand_fb_run"))
    exp_ms = sorted(sum(p[k] for k, _ in kinds) for p in ph)[len(ph) // 2]
    exp_cols = sum(ph[0][k + "_cols"] for k, _ in kinds)
    out_bytes = prog.num_cols * 8 * n
    res = {"workload": f"batch 2^{n.bit_length() - 1} verify_p256_message_circuit fills, 115 557 columns each, curve program (DESIGN.md 5f); "
                       f"{distinct} distinct valid signatures tiled over the batch",
           "value": round(n / med, 1), "unit": "fills/s", "ms_per_call": round(med * 1e3, 3),
           "whole_fill_frac_of_hbm_peak": round(out_bytes / med / 1e9 / HBM_PEAK_GBS, 4),
           "roofline": {"kernel": "kc_expand + kc_expand_runs + kc_expand_fb_run", "bound": "hbm",
                        "algorithmic_bytes": int(exp_cols * 8 * n), "sum_launch_ms": round(exp_ms, 3),
                        "achieved": round(exp_cols * 8 * n / max(exp_ms, 1e-9) / 1e6, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(exp_cols * 8 * n / max(exp_ms, 1e-9) / 1e6 / HBM_PEAK_GBS, 4)}}
    if exp_ms <= 0:   # a context without P2E_CTX_PHASE_TIMING: no per-launch durations
        res["roofline"] = None
    prog.close()
    return res


def cpu_baseline(p2e, seed):
    """Bounded-sample timing of the C oracle on the host cores (checker timed as a baseline only)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_c
    cores = usable_cores(oracle_c.max_threads())
    probe = p2e.synth_signatures(seed=seed, n=4 * cores)
    oracle_c.verify_witness(*[a[:cores] for a in probe], nthreads=cores)   # warm-up (constant tables, threads)
    t = time.time()
    oracle_c.verify_witness(*probe, nthreads=cores)
    rate = len(probe[0]) / max(time.time() - t, 1e-3)
    n = int(min(max(64, rate * 12.0), 20000))                            # sized for ~12 s of CPU work
    sigs = p2e.synth_signatures(seed=seed, n=n)
    t = time.time()
    cols, err, flags = oracle_c.verify_witness(*sigs, nthreads=cores)
    dt = time.time() - t
    assert not err.any() and flags.all()
    base = {"value": round(n / dt, 2), "unit": "fills/s", "cores": cores, "kind": "port",
            "sample": f"{n} signatures of the same synthetic batch, all {cores} host threads (OpenMP), "
                      f"{dt:.1f} s; oracle/p2e_oracle.c (schoolbook mul + Knuth D, one Fermat ladder per inverse)"}
    # variant b: batch inversion across lock-step groups of 256 signatures, everything else unchanged
    group = 256
    t = time.time()
    oracle_c.verify_witness_lockstep(*[a[:group * cores] for a in p2e.synth_signatures(seed=seed, n=group * cores)],
                                     nthreads=cores, group=group)
    rate = group * cores / max(time.time() - t, 1e-3)
    n2 = max(1, int(min(rate * 10.0, 40000) // (group * cores))) * group * cores          # whole groups per thread, ~10 s
    sigs2 = p2e.synth_signatures(seed=seed, n=n2)
    t = time.time()
    cols2, err2, flags2 = oracle_c.verify_witness_lockstep(*sigs2, nthreads=cores, group=group)
    dt2 = time.time() - t
    assert not err2.any() and flags2.all() and (cols2[:, :min(n, n2)] == cols[:, :min(n, n2)]).all()
    opt = {"value": round(n2 / dt2, 2), "unit": "fills/s", "cores": cores, "kind": "port",
           "sample": f"{n2} signatures, {cores} host threads, {dt2:.1f} s; same C code with Montgomery batch inversion "
                     f"across lock-step groups of {group} signatures (one Fermat ladder per group and inverse op); "
                     "columns identical to the faithful variant"}
    return base, opt


def strong_shape(p2e, torch, dist, args, world, rank, dev, dev_index, backend, compact, fill_ms_known=None):
    """BASELINE configs[3] literally: ONE batch of 2^k verifies split over the ranks, the columns assembled on every
    rank.  Measures (a) the fill alone, (b) fill + exchange pipelined block by block (dist.assemble_fill), (c) the
    exchange alone with every block ready.  Times are max over ranks of K steps between barriers."""
    import numpy as np
    from plonky2_ecdsa_amd.dist import ColumnAssembly, assemble_fill, shard_bounds
    total = 1 << args.batch_log2
    start, end = shard_bounds(total, rank, world)
    n = end - start
    n_max = -(-total // world)
    ld = n_max + args.ld_pad + (n_max & 1)
    steps, warmup = max(1, min(args.steps, 10)), max(1, min(args.warmup, 2))
    on_dev = backend == "nccl"
    inputs = [torch.from_numpy(a).to(dev) for a in p2e.synth_signatures(seed=4, n=n, first=start)]
    st = torch.cuda.Stream()
    ctx = p2e.Context(device=dev_index, stream=st.cuda_stream, asynchronous=True)
    err = torch.empty(n, dtype=torch.uint8, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    cmap = None
    if compact:
        cmap, NN, NW = p2e.compact_layout(0)
        shapes = [((NN, ld), torch.int32), ((NW, ld), torch.int64)]
    else:
        shapes = [((p2e.VERIFY_COLS, ld), torch.int64)]
    mats = [torch.empty((world,) + sh, dtype=dt, device=dev if on_dev else "cpu") for sh, dt in shapes]
    asm = ColumnAssembly(mats, total)
    # device assembly: the fill writes straight into this rank's slice of the assembled tensor; host assembly (gloo
    # rehearsal): into a device stage that is copied out block by block
    stage = [asm.local_view(k) for k in range(len(mats))] if on_dev else [torch.empty(sh, dtype=dt, device=dev) for sh, dt in shapes]

    torch.cuda.synchronize()                   # inputs and the zeroed pad column were written on torch's current stream

    def issue():
        if compact:
            ctx.ecdsa_verify_witness_compact_batch(*inputs, narrow=stage[0][:, :n], wide=stage[1][:, :n], err=err, valid=valid,
                                                   ld_narrow=ld, ld_wide=ld)
        else:
            ctx.ecdsa_verify_witness_batch(*inputs, cols=stage[0][:, :n], err=err, valid=valid, ld=ld)

    def barrier():
        dist.barrier()
        torch.cuda.synchronize()

    def timed(body):
        for _ in range(warmup):
            body()
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            ts = time.perf_counter()
            body()
            if os.environ.get("P2E_BENCH_DEBUG"):
                print(f"[rank {rank}] {body.__name__}: {(time.perf_counter() - ts) * 1e3:.3f} ms", file=sys.stderr, flush=True)
        barrier()
        t = torch.tensor([(time.perf_counter() - t0) / steps], dtype=torch.float64, device=dev if on_dev else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def fill_only():
        issue()
        assert ctx.sync() == 0

    def fill_and_assemble():
        segs = assemble_fill(ctx, asm, issue, compact_map=cmap, host_stage=None if on_dev else stage)
        assert ctx.sync() == 0
        torch.cuda.current_stream().synchronize()       # ... and the exchange (asm.wait() made this stream wait for it)
        return segs

    def assemble_only():                       # every block final already: ONE grouped exchange of the whole matrices
        asm.exchange([(0, m.shape[1]) for m in mats])
        asm.wait()
        torch.cuda.current_stream().synchronize()

    t_fill = fill_ms_known / 1e3 if fill_ms_known else timed(fill_only)
    segs = fill_and_assemble()
    t_both = timed(fill_and_assemble)
    assert int(valid.sum()) == n, "synthetic signatures must all verify"
    t_gather = timed(assemble_only)
    # the assembled matrix against this rank's own knowledge of the batch: column 0 of every OTHER rank's shard is limb 0 of
    # its first mul generator's remainder -- cheap spot check of the layout: compare with a fill of that rank's first signatures
    checked = 0
    if rank == 0 and world > 1 and not compact:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle_c
        for r in range(1, world):
            s_r, e_r = shard_bounds(total, r, world)
            k = min(4, e_r - s_r)
            want, _, _ = oracle_c.verify_witness_lockstep(*p2e.synth_signatures(seed=4, n=k, first=s_r))
            got = mats[0][r, :, :k].cpu().numpy().view(np.uint64)
            assert np.array_equal(got, want), f"assembled shard of rank {r} differs from the oracle"
            checked += k
    out = {"what": f"ONE global batch of 2^{args.batch_log2} verifies split over {world} ranks ({n} per GPU); the full "
                   + ("compact container" if compact else "u64 column matrix") + f" assembled on every rank ({backend}: "
                   + ("RCCL grouped send/recv per column block, device to device" if on_dev else "gloo rehearsal through host memory") + ")",
           "batch_per_gpu": n, "fill_ms": round(t_fill * 1e3, 3), "value_fill_only": round(total / t_fill, 1),
           "column_blocks": len(segs), "allgather_alone_ms": round(t_gather * 1e3, 3),
           "fill_plus_allgather_pipelined_ms": round(t_both * 1e3, 3),
           "exposed_allgather_ms": round((t_both - t_fill) * 1e3, 3),
           "value_with_allgather": round(total / t_both, 1),
           "bytes_received_per_rank": int(sum(m[0].numel() * m.element_size() for m in mats) * (world - 1)),
           "GBps_received_per_rank_alone": round(sum(m[0].numel() * m.element_size() for m in mats) * (world - 1) / t_gather / 1e9, 1) if world > 1 else None,
           "assembled_shards_checked_vs_oracle": checked}
    del mats, asm, stage
    ctx.close()
    torch.cuda.empty_cache()
    return out


DUMP_SEED, DUMP_SIGNATURES = 20261015, 32


def dump_outputs(out_dir, torch, n, mats, err, valid):
    """--dump-outputs: the output matrices of one fill restricted to a seeded sample of signatures (every column), and
    the flags of the whole batch.  ``mats``: name -> (columns, >= n) int32 / int64 device matrix.  Every value is
    written as float64, which holds a 32-bit word exactly: 64-bit columns go out as their low and high halves."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    sample = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=min(n, DUMP_SIGNATURES), replace=False))
    idx = torch.from_numpy(sample).to(mats[next(iter(mats))].device)
    arrays = {"err": err.cpu().numpy().astype(np.float32), "valid": valid.cpu().numpy().astype(np.float32)}
    for name, m in mats.items():
        got = m.index_select(1, idx).cpu().numpy()
        if got.dtype == np.int32:
            arrays[name] = got.view(np.uint32).astype(np.float64)
        else:
            got = got.view(np.uint64)
            arrays[name + "_lo32"] = (got & np.uint64(0xFFFFFFFF)).astype(np.float64)
            arrays[name + "_hi32"] = (got >> np.uint64(32)).astype(np.float64)
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def pmc_traffic():
    """HBM bytes per k_expand launch from the committed rocprofv3 PMC summary, if any."""
    best = None
    pdir = os.path.join(ROOT, "profiles")
    if os.path.isdir(pdir):
        for f in sorted(os.listdir(pdir)):
            if f.endswith("_pmc_summary.json"):
                try:
                    best = json.load(open(os.path.join(pdir, f)))
                except Exception:
                    pass
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch-log2", type=int, default=16,
                    help="weak: signatures per GPU = 2^k; strong: signatures of the global batch = 2^k (metric: 16)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--no-strong-leg", action="store_true",
                    help="N>1, weak mode: skip the extra 'strong' object (one global batch of 2^k split over the ranks + assembly)")
    ap.add_argument("--no-limb-split", action="store_true", help="skip the limb-split roofline leg")
    ap.add_argument("--full", action="store_true",
                    help="also the legs that take runs of their own: oracle check of the whole batch, limb-split roofline, "
                         "CPU baselines, P-256 verifier, the strong object at N > 1 (the --no-* options skip single legs)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed to DIR/<name>.npy (see the top of this file)")
    ap.add_argument("--check", type=int, default=None,
                    help="signatures of the last output buffer compared with the oracle, every column "
                         "(default: the whole batch with --full, none otherwise)")
    ap.add_argument("--allgather-cols", type=int, default=0,
                    help="N>1 only: after the timed region, all-gather this many columns over RCCL and report GB/s")
    ap.add_argument("--ld-pad", type=int, default=16, help="column stride = batch + this many elements")
    ap.add_argument("--compact", action="store_true",
                    help="NOT the headline: write the compact container (u32 limb/flag columns + u64 check_sum/carry columns, "
                         "include/p2e.h) instead of the u64 column matrix; same values, 474 KB instead of 661 KB per fill")
    ap.add_argument("--pipeline-depth", type=int, default=1,
                    help="batches in flight per GPU: D > 1 issues step i on context/stream/output buffer i % D "
                         "(asynchronous C ABI), so the scalar phase and first chain pieces of the next batch "
                         "run under the expansion of the current one")
    ap.add_argument("--no-phase-timing", action="store_true",
                    help="contexts without P2E_CTX_PHASE_TIMING: no per-launch HIP events, so no roofline objects on the line; "
                         "what a production caller runs (the events cost 6 %% at 2^13 signatures per call, nothing at 2^16)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-p256", action="store_true", help="skip the P-256 verifier leg (SURVEY 8(f) rank 4 on the driver's line)")
    args = ap.parse_args()
    if args.check is None:
        args.check = 1 << 16 if args.full else 0

    import numpy as np
    import torch
    import torch.distributed as dist
    import plonky2_ecdsa_amd as p2e

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # one process per GPU.  P2E_DIST_BACKEND=gloo is for rehearsing the N>1 code path on a box with fewer
    # GPUs than ranks (ranks then share devices); the driver's runs use the default, nccl (= RCCL over xGMI).
    backend = os.environ.get("P2E_DIST_BACKEND", "nccl")
    dev_index = local_rank % max(1, torch.cuda.device_count())
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{dev_index}"))
        else:
            dist.init_process_group(backend)
    if world != args.gpus and rank == 0:
        print(f"warning: --gpus {args.gpus} but WORLD_SIZE {world}", file=sys.stderr)
    torch.cuda.set_device(dev_index)
    dev = f"cuda:{dev_index}"
    local_rank = dev_index

    from plonky2_ecdsa_amd.dist import shard_bounds
    if args.scaling == "strong":
        total = 1 << args.batch_log2                                       # ONE global batch, split over the ranks
    else:
        total = (1 << args.batch_log2) * world                             # 2^k signatures per GPU
    start, end = shard_bounds(total, rank, world)
    n = end - start
    sigs = p2e.synth_signatures(seed=4, n=n, first=start)                  # seed 0x4: SURVEY.md 8(d) cfg-4
    depth = max(1, args.pipeline_depth)
    # inputs resident in HBM first, then the context: the order a torch caller has (it has touched the GPU before it asks
    # for a context).  Since round 3 the step time does not depend on that order by more than 3 %.
    inputs = [torch.from_numpy(a).to(dev) for a in sigs]
    torch.cuda.synchronize()
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(depth - 1)]
    # (phase_timing: the per-launch HIP events the roofline objects are computed from)
    ctxs = [p2e.Context(device=local_rank, stream=st.cuda_stream, asynchronous=depth > 1, phase_timing=not args.no_phase_timing) for st in streams]
    ctx = ctxs[0]
    # column stride: n + 16 elements.  A power-of-two stride (2^16 * 8 B = 512 KiB) makes consecutive columns
    # camp on the same HBM channels (measured -9 % on k_expand); ld is part of the C ABI (ld >= n).
    ld = n + args.ld_pad
    if args.compact:
        _m, NN, NW = p2e.compact_layout(0)
        nar_bufs = [torch.empty((NN, ld), dtype=torch.int32, device=dev) for _ in range(depth)]
        wid_bufs = [torch.empty((NW, ld), dtype=torch.int64, device=dev) for _ in range(depth)]
        cols_bufs = [None] * depth
        cols = None
    else:
        cols_bufs = [torch.empty((p2e.VERIFY_COLS, ld), dtype=torch.int64, device=dev) for _ in range(depth)]
        cols = cols_bufs[0][:, :n]
    errs = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(depth)]
    valids = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(depth)]
    err, valid = errs[0], valids[0]
    issued = [0]

    def step():
        k = issued[0] % depth
        issued[0] += 1
        if depth > 1 and issued[0] > depth:
            ctxs[k].sync()                     # the batch issued `depth` steps ago on this context is done
        if args.compact:
            return ctxs[k].ecdsa_verify_witness_compact_batch(*inputs, narrow=nar_bufs[k], wide=wid_bufs[k], err=errs[k],
                                                              valid=valids[k], ld_narrow=ld, ld_wide=ld)[4]
        return ctxs[k].ecdsa_verify_witness_batch(*inputs, cols=cols_bufs[k][:, :n], err=errs[k], valid=valids[k], ld=ld)[3]

    def drain():
        bad = 0
        for c in ctxs:
            bad += c.sync() if depth > 1 else 0
        return bad

    for _ in range(args.warmup):
        bad = step()
    bad = (drain() if depth > 1 else bad) if args.warmup else 0
    torch.cuda.synchronize()
    if args.warmup:
        assert bad == 0 and all(int(v.sum()) == n for v in valids[:min(depth, args.warmup)]), "synthetic signatures must all verify"
    issued[0] = 0

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    kstat = {k: {"ms": [], "cols": 0.0, "launches": 0} for k in ("expand", "runs", "fbrun")}
    phase_acc = {}

    def note(ph, weight=1.0):
        for k, st in kstat.items():
            st["ms"].append(ph[k])
            st["cols"], st["launches"] = ph[k + "_cols"], int(ph[k + "_launches"])
        for k in ("scalar", "expand", "runs", "fbrun", "total"):
            phase_acc[k] = phase_acc.get(k, 0.0) + ph[k] * weight
    step_s = []
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ts = time.perf_counter()
        step()
        if depth > 1:
            continue
        step_s.append(time.perf_counter() - ts)      # calls are synchronous at depth 1: the step's own wall time
        note(ctx.last_phase_ms())
    if depth > 1:
        drain()
    barrier()
    elapsed = time.perf_counter() - t0
    if depth > 1:                              # per-launch timings of the last batch of every context
        for c in ctxs:
            note(c.last_phase_ms(), args.steps / depth)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    gather = None
    if world > 1 and args.allgather_cols > 0 and not args.compact and args.scaling == "weak":
        from plonky2_ecdsa_amd.dist import all_gather_columns
        k = min(args.allgather_cols, p2e.VERIFY_COLS)
        barrier()
        tg = time.perf_counter()
        g = all_gather_columns(cols[:k] if backend == "nccl" else cols[:k].cpu(), total)
        barrier()
        tg = time.perf_counter() - tg
        gather = {"cols": k, "bytes_per_rank_out": int(g.numel() * 8), "ms": round(tg * 1e3, 3),
                  "GBps_per_rank": round(g.numel() * 8 / tg / 1e9, 1)}
        del g

    if rank == 0 and args.dump_outputs:
        k = (issued[0] - 1) % depth                    # the buffer set the last timed step wrote
        if args.compact:
            mats = {"narrow": nar_bufs[k], "wide": wid_bufs[k]}
        else:
            mats = {"columns": cols_bufs[k]}
        dump_outputs(args.dump_outputs, torch, n, mats, errs[k], valids[k])

    checked = None
    if rank == 0 and args.check > 0 and args.compact:
        # the compact container of THIS run against the oracle: sampled signatures, every column
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle_c
        k = (issued[0] - 1) % depth if issued[0] else 0
        sample = np.unique(np.linspace(0, n - 1, min(args.check, n, 4096)).astype(np.int64))
        want, werr, wflags = oracle_c.verify_witness_lockstep(*[a[sample] for a in sigs], nthreads=usable_cores(oracle_c.max_threads()))
        idx = torch.from_numpy(sample).to(dev)
        got = p2e.compact_expand(0, nar_bufs[k][:, idx].cpu().numpy().view(np.uint32), wid_bufs[k][:, idx].cpu().numpy())
        assert np.array_equal(got, want) and not werr.any() and wflags.all(), "GPU compact container differs from the oracle"
        checked = int(len(sample))
    if rank == 0 and args.check > 0 and not args.compact:
        # bit-exactness of THIS run: sampled signatures of the last output buffer against the C oracle, every column
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle_c
        last = cols_bufs[(issued[0] - 1) % depth] if issued[0] else cols_bufs[0]
        cores = usable_cores(oracle_c.max_threads())
        if args.check >= n:
            # the whole batch: contiguous chunks through the oracle's lock-step walk (bit-identical to the faithful walk,
            # tests/test_oracle.py::test_optimised_cpu_variant_is_bit_identical), compared on the GPU
            checked = 0
            for a in range(0, n, 4096):
                b = min(n, a + 4096)
                want, werr, wflags = oracle_c.verify_witness_lockstep(*[x[a:b] for x in sigs], nthreads=cores)
                assert not werr.any() and wflags.all()
                assert torch.equal(last[:, a:b], torch.from_numpy(want.view(np.int64)).to(dev)), \
                    f"GPU columns differ from the oracle in signatures [{a}, {b})"
                checked += b - a
        else:
            sample = np.unique(np.linspace(0, n - 1, min(args.check, n)).astype(np.int64))
            want, werr, wflags = oracle_c.verify_witness_lockstep(*[a[sample] for a in sigs], nthreads=cores)
            got = last[:, torch.from_numpy(sample).to(dev)].cpu().numpy().view(np.uint64)
            assert np.array_equal(got, want) and not werr.any() and wflags.all(), "GPU columns differ from the oracle"
            checked = int(len(sample))

    strong = None
    if world > 1 and (args.scaling == "strong" or (args.full and not args.no_strong_leg)):
        # free this leg's output buffers first: the assembled tensor is another (world, cols, ld) matrix
        keep_ms = elapsed / args.steps * 1e3 if (args.scaling == "strong" and depth == 1) else None
        cols_bufs.clear()
        if args.compact:
            nar_bufs.clear()
            wid_bufs.clear()
        cols = None
        torch.cuda.empty_cache()
        try:
            strong = strong_shape(p2e, torch, dist, args, world, rank, dev, dev_index, backend, args.compact, fill_ms_known=keep_ms)
        except Exception as e:      # the headline line (the timed region above) must survive this leg
            strong = {"error": f"{type(e).__name__}: {e}"}

    limb_split = None
    if rank == 0 and args.full and not args.no_limb_split:
        # the 29-bit limb-split kernel of the north star (>= 40 % of HBM peak asked): 2^26 packed values -> 9 limb columns
        m = 1 << 26
        packed = torch.randint(0, 256, (m, 32), dtype=torch.uint8, device=dev)
        limbs = torch.empty((9, m), dtype=torch.int64, device=dev)
        for _ in range(2):
            ctx.limb_split(packed, out=limbs)
        reps = 10
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        torch.cuda.synchronize()
        ev[0].record()
        for k in range(reps):                          # the context runs on torch's current stream: the events see it
            ctx.limb_split(packed, out=limbs)
            ev[k + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[k].elapsed_time(ev[k + 1]) for k in range(reps))
        med = ms[len(ms) // 2]
        # one spot check of the split itself
        v = int.from_bytes(bytes(packed[12345].cpu().numpy()), "little")
        assert [int(x) for x in limbs[:, 12345].cpu()] == [(v >> (29 * k)) & ((1 << 29) - 1) for k in range(9)]
        ach = 104 * m / (med / 1e3) / 1e9
        limb_split = {"kernel": "k_split", "bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                      "frac": round(ach / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_launch": 104 * m,
                      "avg_launch_ms": round(med, 4), "elements": m, "traffic": None,
                      "note": "median of 10 launches incl. the call's own stream sync; 104 B/element (32 packed in + 9 x 8 out)"}
        del packed, limbs

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = total * args.steps / elapsed
        # the committed PMC summary was collected on the metric's batch (2^16 per GPU): no traffic figure otherwise
        pmc = (pmc_traffic() or {}) if (args.batch_log2 == 16 and args.scaling == "weak") else {}

        def roofline(kernel, st):
            # `launches` launches per step (one per schedule segment); per launch:
            if not st["launches"] or args.no_phase_timing:
                return None
            avg_s = sum(st["ms"]) / len(st["ms"]) / 1e3 / st["launches"]
            alg_bytes = int(st["cols"]) * 8 * n // st["launches"]
            achieved = alg_bytes / avg_s / 1e9
            return {"kernel": kernel, "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_launch": alg_bytes,
                    "avg_launch_ms": round(avg_s * 1e3, 4), "launches_per_step": st["launches"],
                    "cols_per_fill_all_launches": int(st["cols"]),
                    "traffic": (pmc.get("hbm_bytes_per_launch") or {}).get(kernel),
                    "traffic_source": pmc.get("source")}

        runs_line, expand_line = roofline("k_expand_runs", kstat["runs"]), roofline("k_expand", kstat["expand"])
        fbrun_line = roofline("k_expand_fb_run", kstat["fbrun"])
        bytes_per_fill = BYTES_PER_FILL
        if args.compact:   # the per-kernel byte counts above assume 8-byte columns: not quoted for this container
            runs_line = expand_line = fbrun_line = None
            bytes_per_fill = 160 + NN * 4 + NW * 8
        line = {
            "metric": "secp256k1 ECDSA witness fills/sec at batch=2^16, 1/2/4/8 MI355X; bit-exact",
            "value": round(value, 1), "unit": "fills/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": args.scaling,
            "vs_baseline": None, "dtype": "u64", "data": "synthetic",
            "config": {"workload": (f"ONE global batch of 2^{args.batch_log2} ECDSA verifies split over the ranks "
                                    "(BASELINE configs[3], the metric's literal shape)" if args.scaling == "strong" else
                                    f"batch 2^{args.batch_log2} ECDSA verifies per GPU (BASELINE configs[3] workload on one GPU)")
                                   + "; random valid signatures, seed 4; all 82615 hot-path generator columns, "
                                   "column-major u64 (Goldilocks) in HBM; witness arithmetic in 8 x u32 limbs, curve chains and inversion batches in 9 unsaturated 29-bit limbs",
                       "container": "compact (u32 narrow + u64 wide matrices), NOT the headline format" if args.compact
                                    else "u64 column matrix",
                       "batch_per_gpu": n, "global_batch": total, "cols_per_fill": p2e.VERIFY_COLS, "ld": ld,
                       "pipeline_depth": depth,
                       "parallelism": f"shard{world}" if world > 1 else "single"},
            "whole_fill": {"algorithmic_bytes_per_fill": bytes_per_fill,
                           "GBps_per_gpu": round(value * bytes_per_fill / world / 1e9, 1),
                           "frac_of_hbm_peak": round(value * bytes_per_fill / world / 1e9 / HBM_PEAK_GBS, 4)},
            "phase_ms_per_step": {k: round(v / args.steps, 4) for k, v in phase_acc.items()},
            # P2E_RUN_ITERS=0 expands everything op by op: k_expand is then the only expansion kernel
            "roofline": runs_line or expand_line,
        }
        if runs_line:
            line["roofline_k_expand"] = expand_line
        if fbrun_line:
            line["roofline_k_expand_fb_run"] = fbrun_line
        if step_s:
            med = sorted(step_s)[len(step_s) // 2]
            line["median_step_ms"] = round(med * 1e3, 4)            # median of the timed steps
            line["value_at_median_step"] = round(n / med, 1) if world == 1 else None
        if limb_split:
            line["roofline_limb_split"] = limb_split
        if checked is not None:
            line["checked_vs_oracle"] = checked
        if gather:
            line["allgather"] = gather
        if strong:
            line["strong"] = strong
            if args.scaling == "strong" and "value_with_allgather" in strong:
                line["value_with_allgather"] = strong["value_with_allgather"]
        if world == 1 and args.full and not args.no_cpu_baseline:
            line["cpu_baseline"], line["cpu_baseline_optimised"] = cpu_baseline(p2e, seed=4)
        if world == 1 and args.full and not args.no_p256 and not args.compact and args.batch_log2 == 16:
            try:
                cols_bufs.clear()
                torch.cuda.empty_cache()
                line["p256_verify"] = p256_leg(p2e, torch, ctx, dev, n)
            except Exception as e:   # the headline line must survive this leg
                line["p256_verify"] = {"error": f"{type(e).__name__}: {e}"}
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
