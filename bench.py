#!/usr/bin/env python3
"""bench.py -- self-play hot-path throughput on MI355X (metric of BASELINE.json).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A "step" is one lock-step ROUND of the hot path over every concurrent game of the rank:
the tree kernels (hand-written HIP: backup / PUCT select / expand / game rules, leaf planes into the queue) followed by
one ResNet forward over the evaluation queue.  Workload at N=1 = BASELINE.json configs[1] ("normal"):
4096 concurrent games per GPU, 800 sims/move, 7-block x 128-filter net, random-init weights, synthetic self-play
from the opening position.  Games shard across ranks (disjoint game ids, no data-path collective); RCCL is used
only to all-reduce the counters.  `--gpus N` without a launcher re-executes itself under torch.distributed.run.
Rank 0 prints ONE JSON line: the timed steps (`value`) and the roofline of the dominant kernel measured with HIP
events on its stream during those steps.  A plain run does nothing else: it sets up, warms up, times the steps, writes
--dump-outputs and prints the line.  `--full` adds, in the same invocation: at N=1 a sustained leg of 3000 more rounds
(`sustained` / `value_sustained`: games in every phase, finished games replaced, measured plies/s and games/hour, tree
memory, tree_resets), the numerics check of the network against the fp32 PyTorch module, the short legs of the other
BASELINE configurations (`other_configs`), the rule-kernel micro-suite and the CPU baseline (the C port of the
reference's tree + rules on every CPU the container may use).  `--config eval` times the evaluator arena on the arena
worker instead.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "chinesechess-alphazero_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def _load_profile(path):
    """A committed profile: a JSON document, or a bench line (first line of the file).  None when unreadable -- a
    damaged evidence file must never break the benchmark itself."""
    try:
        with open(path) as f:
            text = f.read()
        try:
            return json.loads(text)
        except ValueError:
            return json.loads(text.splitlines()[0])
    except (OSError, ValueError, IndexError):
        return None


class _stdout_to_stderr:
    """RCCL prints a version banner on stdout (at communicator set-up or tear-down, depending on NCCL_DEBUG): while this
    is active file descriptor 1 points at stderr, so that rank 0's stdout carries the ONE JSON line and nothing else."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        return False


FULL_RECORD = "bench_full.json"
COMPACT_LIMIT = 4096


def _r(x, digits=6):
    """floats of the compact line: 6 significant digits"""
    return float(f"{x:.{digits}g}") if isinstance(x, float) else x


def compact_line(out):
    """The ONE stdout line (the driver parses the last stdout line and its reader is bounded -- round 4's
    30 KB line came back `parsed: null`): the contract's keys, `roofline` and `cpu_baseline` with short strings only, and the
    handful of scalars a reader needs beside them.  Everything else (other_configs, guard report, tree shape, sustained
    detail, micro-suite, the long kernel descriptions) goes to bench_full.json next to this script (+ gpurun_out/) and to
    stderr.  Kept below COMPACT_LIMIT bytes (tests/test_host_logic.py::test_bench_line_is_compact)."""
    def pick(d, keys):
        return {k: _r(d[k]) for k in keys if d is not None and k in d and d[k] is not None}
    c = {k: _r(out.get(k)) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                      "higher_is_better", "scaling", "vs_baseline", "dtype", "data")}
    if out.get("per_rank_value") is not None:
        c["per_rank_value"] = [_r(float(v)) for v in out["per_rank_value"]]
    cfg = out.get("config") or {}
    c["config"] = pick(cfg, ("workload", "games_per_gpu", "games", "sims_per_round", "queue_slots_per_gpu", "parallelism"))
    if "workload" in c["config"]:
        c["config"]["workload"] = c["config"]["workload"][:200]
    rf = out.get("roofline")
    c["roofline"] = None
    if rf:
        c["roofline"] = pick(rf, ("bound", "achieved", "peak", "unit", "frac", "avg_launch_ms", "launches_timed",
                                  "traffic", "traffic_source", "boards_per_launch", "mfma_util_pmc"))
        c["roofline"]["kernel"] = str(rf.get("kernel_short") or rf.get("kernel", ""))[:80]
        c["roofline"].setdefault("traffic", None)
    rs = out.get("roofline_search")
    if rs and rs is not rf:
        c["roofline_search"] = pick(rs, ("bound", "achieved", "peak", "unit", "frac", "avg_launch_ms", "traffic"))
    cb = out.get("cpu_baseline")
    if cb:
        c["cpu_baseline"] = pick(cb, ("value", "unit", "cores", "kind", "cpu_model"))
        c["cpu_baseline"]["sample"] = str(cb.get("sample", ""))[:160]
        wn = (cb.get("with_network_estimate") or {}).get("value")
        if wn is not None:
            c["cpu_baseline"]["with_network_estimate"] = _r(float(wn))
        rp = cb.get("reference_python")
        if rp:                                              # the UNMODIFIED reference (Python), timed where it exists (build container)
            c["cpu_baseline"]["reference_python"] = rp
    else:
        c["cpu_baseline"] = None
    for k in ("value_sustained", "roofline_frac_sustained", "games_per_hour_steady_state", "net_arith_requested",
              "net_arith_effective", "numerics_logit_max_abs", "numerics_within_tolerance", "numerics_peaked_arith",
              "numerics_peaked_policy_max_abs", "value_peaked_policy", "roofline_frac_peaked_policy"):
        if out.get(k) is not None:
            c[k] = _r(out[k])
    sus = out.get("sustained") or {}
    if sus:
        c["sustained"] = pick(sus, ("rounds", "seconds", "ms_per_step", "games_finished", "queue_utilisation",
                                    "search_round_ms", "search_round_ms_max", "tree_resets"))
    oc = out.get("other_configs") or {}
    if oc:                                                   # one number per leg: expansions/s (None = the leg failed)
        c["other_configs_exp_per_s"] = {k: (_r(float(v["value"])) if isinstance(v, dict) and "value" in v else None)
                                        for k, v in oc.items()}
    ms = out.get("micro_suite") or {}
    if ms:
        c["micro_suite"] = pick(ms, ("achieved", "unit", "frac", "ms", "boards"))
    col = out.get("collective") or {}
    if col:
        c["collective"] = pick(col, ("backend", "world", "all_reduce_int64x8_us", "probe_ok"))
    c["full_record"] = FULL_RECORD
    return c


def emit(out):
    """rank 0: the full record to bench_full.json (next to the script, and into gpurun_out/ when that exists) and to
    stderr; the compact line -- and nothing else -- to stdout, last."""
    text = json.dumps(out)
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        if os.path.isdir(d):
            try:
                with open(os.path.join(d, FULL_RECORD), "w") as f:
                    f.write(text + "\n")
            except OSError as e:
                print(f"bench.py: could not write {d}/{FULL_RECORD}: {e}", file=sys.stderr)
    if os.environ.get("CZ_BENCH_FULL_LINE") == "1":
        # the repository's own profiling scripts (tools/*.sh, tools/summarize_profiles.py) read every key from the stdout
        # line; the driver never sets this
        print(text, flush=True)
        return
    print("[bench full record] " + text, file=sys.stderr, flush=True)
    c = compact_line(out)
    line = json.dumps(c, separators=(",", ":"))
    # a line the driver cannot parse is an unmeasured round: drop optional groups before ever exceeding the limit
    for k in ("collective", "micro_suite", "sustained", "other_configs_exp_per_s", "roofline_search"):
        if len(line) <= COMPACT_LIMIT:
            break
        c.pop(k, None)
        line = json.dumps(c, separators=(",", ":"))
    sys.stderr.flush()
    print(line, flush=True)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--config", default="normal", choices=["mini", "normal", "deep", "eval"])
    ap.add_argument("--arith", default=None,
                    help="REQUESTED products of the float32 tower (default: the config's engine.net_arith = c6: fp16 + two bf6 correction MFMAs): c8 = fp16 "
                         "main term + two scaled-fp8 correction MFMAs, c8>N = the first N blocks on c8, f16x3 / bf16x3 = three "
                         "MFMAs on (hi, lo) fp16 / bf16 pairs.  The engine measures the request against float64 when it loads "
                         "the weights and may fall back (net_arith_effective in the line)")
    ap.add_argument("--games", type=int, default=None, help="concurrent games per GPU (default: config)")
    ap.add_argument("--sims-per-round", type=int, default=None, help="K, lock-step batch per game")
    ap.add_argument("--dtype", default=None, choices=["float32", "bfloat16", "float16"])
    ap.add_argument("--trunk", default=None, choices=["mfma", "library"],
                    help="residual tower: hand-written MFMA convolution (default) or MIOpen")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check what the headline figure does not need: the "
                         "sustained leg, the numerics check, other_configs, the micro-suite and the CPU baseline (the "
                         "--no-* options below leave out single parts of it)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-micro", action="store_true", help="skip the 1M-board rule-kernel micro-suite")
    ap.add_argument("--cpu-baseline-seconds", type=float, default=12.0)
    ap.add_argument("--graph", action="store_true", help="replay each round from a HIP graph")
    ap.add_argument("--plain-resblock", action="store_true",
                    help="A/B: residual blocks on k_resblock instead of the software-pipelined k_resblock_pipe")
    ap.add_argument("--sustained-rounds", type=int, default=None,
                    help="rounds of the sustained leg that follows the timed steps (default 3000 with --full at N=1 "
                         "for the 'normal' config, 0 otherwise)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short legs of the other single-GPU BASELINE configurations (other_configs)")
    ap.add_argument("--other-config-seconds", type=float, default=6.0, help="timed seconds per other_configs leg")
    ap.add_argument("--no-dist", action="store_true",
                    help="N = 1 only: do not initialise torch.distributed (by default a single rank also brings RCCL "
                         "up and runs the counter all-reduce, so that the collective path executes on one GPU)")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU: only the launch / barrier / counter all-reduce plumbing of the ranks (gloo), with "
                         "synthetic counters; used by the CPU test of --gpus N")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (rank 0) as DIR/<name>.npy "
                         "(float32 / float64, a fixed sample where an output is large): two builds run with the same "
                         "arguments can then be compared output for output")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def extra_legs(args, world):
    """What a self-play run does after its timed steps besides --dump-outputs.  A plain run: nothing, unless
    --sustained-rounds asks for a sustained leg.  --full: the sustained leg (3000 rounds by default at N=1 for the
    'normal' config without --graph), the numerics check, and at N=1 other_configs ('normal' config only), the
    micro-suite and the CPU baseline, each unless its --no-* option is given."""
    n_sus = args.sustained_rounds
    if n_sus is None:
        n_sus = 3000 if (args.full and world == 1 and args.config == "normal" and not args.graph) else 0
    one = args.full and world == 1
    return {"sustained_rounds": n_sus, "numerics_check": args.full,
            "other_configs": one and args.config == "normal" and not args.no_other_configs,
            "micro_suite": one and not args.no_micro, "cpu_baseline": one and not args.no_cpu_baseline}


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: re-exec this script under torch.distributed.run with one rank per
    GPU (the same command the driver uses; reference shape: worker/self_play.py:55-60, one worker per device).
    Returns the launcher's exit code."""
    import socket
    import subprocess
    if not args.dry_run:
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            print(f"bench.py: --gpus {args.gpus} but only {have} GPU(s) are visible", file=sys.stderr)
            return 2
    with socket.socket() as sk:                     # a free rendezvous port on the loopback interface
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def init_collective(world, rank, args):
    """torch.distributed over RCCL (backend "nccl"), also for ONE rank: the games never exchange data, the only
    collective of the path is the all-reduce of the counter vector (reference worker/self_play.py:55-60), and
    with a single rank it still goes through RCCL's communicator set-up and a real all-reduce launch -- so the code the
    driver's 8-GPU run depends on executes on every 1-GPU run too.  Returns a record for the JSON line.  At world = 1 a
    failing RCCL is reported, not fatal (the games do not need it)."""
    if world == 1 and args.no_dist:
        return {"backend": None, "world": 1, "note": "--no-dist"}
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if "MASTER_PORT" not in os.environ:                  # no launcher: a single rank on a free loopback port
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    t0 = time.perf_counter()
    try:
        with _stdout_to_stderr():
            dist.init_process_group("nccl", rank=rank, world_size=world)
            probe = torch.ones(8, dtype=torch.int64, device="cuda")
            dist.all_reduce(probe, op=dist.ReduceOp.SUM)          # creates the communicator
            torch.cuda.synchronize()
            ok = bool((probe == world).all())
            init_s = time.perf_counter() - t0
            dist.barrier()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(20):
                dist.all_reduce(probe, op=dist.ReduceOp.MAX)
            torch.cuda.synchronize()
            us = (time.perf_counter() - t1) / 20 * 1e6
            return {"backend": dist.get_backend(), "world": dist.get_world_size(), "init_seconds": init_s,
                    "all_reduce_int64x8_us": us, "probe_ok": ok,
                    "launched_by": "torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ or "LOCAL_RANK" in os.environ
                    else "bench.py itself (single rank)"}
    except Exception as e:                                    # noqa: BLE001
        if world > 1:
            raise
        if dist.is_initialized():
            dist.destroy_process_group()
        return {"backend": None, "world": 1, "error": f"{type(e).__name__}: {e}"[:300]}


def dry_run(args, world, rank):
    """The multi-rank plumbing without an engine: every rank contributes a known counter vector; rank 0 prints the
    line with n_gpus = the number of ranks that actually reported."""
    dist.init_process_group("gloo", rank=rank, world_size=world) if world > 1 else None
    delta = torch.tensor([1000 * (rank + 1), 1], dtype=torch.int64)      # expansions, ranks reporting
    tmax = torch.tensor([0.5 + 0.1 * rank], dtype=torch.float64)
    if world > 1:
        dist.barrier()
        dist.all_reduce(delta, op=dist.ReduceOp.SUM)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    mine = torch.zeros(world, dtype=torch.float64)
    mine[rank] = 1000.0 * (rank + 1) / (0.5 + 0.1 * rank)
    if world > 1:
        dist.all_reduce(mine, op=dist.ReduceOp.SUM)
    if rank == 0:
        secs = tmax.item()
        emit({"metric": "mcts_node_expansions_per_sec", "value": delta[0].item() / secs,
              "unit": "expansions/s", "n_gpus": int(delta[1].item()), "per_rank_value": mine.tolist(), "steps": args.steps,
              "warmup": args.warmup, "ms_per_step": secs / max(1, args.steps) * 1e3, "higher_is_better": True,
              "scaling": "weak", "vs_baseline": None, "dtype": "none (dry run)",
              "data": "dry-run (no GPU work: launch plumbing only)",
              "config": {"workload": "dry run: synthetic counters through the rank launch / barrier / all-reduce plumbing",
                         "games_per_gpu": 0, "sims_per_round": 0, "parallelism": f"{world} rank(s), gloo"},
              "roofline": None, "cpu_baseline": None})
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def build_config(args):
    from cchess_alphazero.config import Config
    from cchess_alphazero.configs._tables import benchmark_overrides
    cfg = Config("normal")
    m, p, e = benchmark_overrides(args.config)
    for k, v in m.items():
        setattr(cfg.model, k, v)
    for k, v in p.items():
        setattr(cfg.play, k, v)
    for k, v in e.items():
        setattr(cfg.engine, k, v)
    if args.games:
        cfg.engine.games_per_gpu = args.games
    if args.sims_per_round:
        cfg.play.search_threads = args.sims_per_round
    if args.dtype:
        cfg.engine.net_dtype = args.dtype
    if args.trunk:
        cfg.engine.net_trunk = args.trunk
    return cfg


def cpu_baseline(cfg, seconds):
    """CPU leg (kind "port"): the C restatement of the reference's player.py + static_env.py (oracle/) on EVERY host
    core at once -- P = usable cores independent processes, one seed each, a new tree per game, same search
    parameters, network replaced by the hash stub (tree + rules only, like BASELINE.md section 2).  The reference's
    own Python path cannot run on the GPU box (/root/reference is not there); its timing on the build container is
    in profiles/r*_reference_cpu.json.  Not like-for-like with the GPU line (which includes the 7x128 network)."""
    import statistics
    import subprocess
    pc = cfg.play
    procs = len(os.sched_getaffinity(0))
    quota = None
    try:                                                     # a container may be allowed fewer CPUs than it can see
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        pass
    visible = procs
    if quota is not None and quota >= 1:
        procs = min(procs, int(quota + 0.999))               # one process per CPU the container may actually use
    cmd = [sys.executable, os.path.join(ROOT, "oracle", "baseline_worker.py"), "--procs", str(procs),
           "--seconds", str(seconds), "--sims", str(pc.simulation_num_per_move), "--threads", str(pc.search_threads),
           "--c-puct", str(pc.c_puct), "--vl", str(pc.virtual_loss), "--max-game-length", str(pc.max_game_length)]
    d = json.loads(subprocess.check_output(cmd, timeout=seconds * 6 + 120))
    per = [r["expansions_per_s"] for r in d["per_process"]]
    sims = [r["sims_per_s"] for r in d["per_process"]]
    cpu = "?"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next(line.split(":", 1)[1].strip() for line in f if line.startswith("model name"))
    except (OSError, StopIteration):
        pass
    net_cpu = cpu_network_rate(cfg, procs)
    combined = None
    if net_cpu and net_cpu.get("positions_per_s"):
        combined = 1.0 / (1.0 / sum(per) + 1.0 / net_cpu["positions_per_s"])
    return {"value": sum(per), "unit": "expansions/s", "cores": procs, "kind": "port",
            "network_on_the_same_cores": net_cpu,
            "with_network_estimate": {"value": combined, "unit": "expansions/s",
                                      "note": "tree + rules (value) and the network evaluation of every expansion "
                                              "(network_on_the_same_cores) taking turns on the same cores: 1 / (1 / tree "
                                              "rate + 1 / network rate) -- the like-for-like figure next to the GPU line, "
                                              "which includes the network"},
            "per_process": {"median": statistics.median(per), "min": min(per), "max": max(per), "seeds": len(per)},
            "sims_per_s": sum(sims), "cpu_model": cpu, "cgroup_cpu_quota": quota, "cpus_visible": visible,
            "sample": f"oracle/xq_mcts.c + xq_rules.c (C port of player.py / static_env.py), {procs} processes x "
                      f"{seconds:.0f} s of self-play from INIT_STATE, {pc.simulation_num_per_move} sims/move, "
                      f"K={pc.search_threads}, hash-stub net (tree + rules only, no ResNet), one seed per process, "
                      f"new tree per game; value = sum over processes",
            "reference_python_timing": reference_cpu_timing(), "reference_python": reference_python_compact()}


def cpu_network_rate(cfg, threads, seconds=3.0):
    """The policy/value network of the benchmarked configuration as a plain PyTorch fp32 module on the host cores the
    container may use: positions per second on batches of 256 (a few seconds).  The CPU leg above has no network in it;
    this is what its expansions would additionally cost on the same machine."""
    try:
        from cchess_alphazero.agent.model import CChessNet
        old = torch.get_num_threads()
        torch.set_num_threads(max(1, int(threads)))
        torch.manual_seed(0)
        net = CChessNet.from_model_config(cfg.model).eval()
        x = (torch.rand((256, 14, 10, 9)) < 0.1).float()
        with torch.no_grad():
            net(x)
            t0 = time.perf_counter()
            n = 0
            while time.perf_counter() - t0 < seconds:
                net(x)
                n += x.shape[0]
            dt = time.perf_counter() - t0
        torch.set_num_threads(old)
        return {"positions_per_s": n / dt, "threads": int(threads), "batch": 256,
                "what": f"{cfg.model.res_layer_num}x{cfg.model.cnn_filter_num} CChessNet, PyTorch CPU fp32"}
    except Exception as e:                                    # noqa: BLE001
        return {"positions_per_s": None, "error": f"{type(e).__name__}: {e}"[:200]}


def reference_cpu_timing():
    """The unmodified reference (Python/NumPy) timed on the build container (it does not exist on the GPU box):
    summary of the committed profiles/r*_reference_cpu.json, SURVEY 8(d)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_reference_cpu.json")))
    if not files:
        return None
    d = _load_profile(files[-1])
    if d is None:
        return None
    out = {"source": os.path.relpath(files[-1], ROOT)}
    for k in ("host", "summary"):
        if k in d:
            out[k] = d[k]
    return out


def reference_python_compact():
    """cpu_baseline.reference_python of the compact line: the unmodified reference's own figure -- value,
    host, cores, K -- from the committed timing (profiles/r*_reference_cpu.json: SURVEY 8(d)'s protocol, stub network, the
    reference's default search_threads), next to the C port's."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_reference_cpu.json")))
    d = _load_profile(files[-1]) if files else None
    if not d:
        return None
    runs = [r for r in d.get("runs", []) if r.get("network") == "stub"]
    if not runs:
        return None
    r = max(runs, key=lambda x: x.get("aggregate_expansions_per_s_median", 0.0))
    return {"value": _r(float(r["aggregate_expansions_per_s_median"])), "unit": "expansions/s", "network": "stub",
            "search_threads": r.get("search_threads"), "processes": r.get("processes"),
            "cores": (d.get("host") or {}).get("cpus"), "host": str((d.get("host") or {}).get("model", ""))[:48],
            "source": os.path.relpath(files[-1], ROOT)}


def micro_suite(n=1 << 20, iters=10):
    """SURVEY 8(d) micro-suite: move-gen + done(need_check) + planes for 1 M boards (the fixed 1k-position suite
    replicated), 90 B in, 256 + 6 + 5040 B out per board: the rule kernel where an HBM fraction is meaningful."""
    from cchess_alphazero import _native
    from cchess_alphazero.environment.static_env import state_to_array
    import numpy as np
    with open(os.path.join(ROOT, "tests", "golden", "positions_1k.json")) as f:
        states = [r["state"] for r in json.load(f)["positions"]]
    base = torch.from_numpy(np.stack([state_to_array(s) for s in states])).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    boards = base[torch.randint(0, base.shape[0], (n,), device="cuda", generator=g)].contiguous()
    out = _native.rules_fused(boards, _native.F32)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        _native.rules_fused(boards, _native.F32, out=out)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / iters
    bytes_per_board = 90 + 256 + 6 + 5040
    gbs = n * bytes_per_board / (ms * 1e-3) / 1e9
    return {"kernel": "k_rules_tpb<f32> (cz_rules_fused dispatches to the lane-per-board kernel at this size)", "boards": n, "bytes_per_board": bytes_per_board, "ms": ms,
            "boards_per_s": n / (ms * 1e-3), "achieved": gbs, "peak": 8000.0, "unit": "GB/s", "frac": gbs / 8000.0}


def games_per_hour_estimate(expansions_per_s, config):
    """games/hour = expansions/s / (mean expansions per finished game) * 3600.  No game finishes inside a
    short benchmark window (a game is ~10^4 rounds), so the per-game cost comes from a complete-games run of the
    same search configuration (tools/measure_games.py -> profiles/r*_games_<config>.json)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_games_{config}.json")))
    if not files:
        return None
    d = _load_profile(files[-1])
    if d is None or "expansions_per_game" not in d:
        return None
    out = {"value": expansions_per_s / d["expansions_per_game"] * 3600.0, "unit": "games/hour",
           "expansions_per_game": d["expansions_per_game"], "mean_plies_per_game": d["mean_plies_per_game"],
           "source": os.path.relpath(files[-1], ROOT)}
    # the sustained figure of the committed long run of this configuration (games in every phase), if there is one
    longs = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_f32_*_rounds.json")),
                   key=lambda f: (int(f.split("_")[-2]), os.path.basename(f)))   # longest run, newest round
    ld = _load_profile(longs[-1]) if (config == "normal" and longs) else None
    if ld is not None:
        sl = ld.get("sustained") or {"plies_per_s": ld["plies_per_s"], "value": ld["value"], "rounds": ld["steps"],
                                      "games_finished": ld["games_finished"]}      # (round-1 files: the whole run)
        out["sustained_measured"] = {"games_per_hour": sl["plies_per_s"] / d["mean_plies_per_game"] * 3600.0,
                                     "expansions_per_s": sl["value"], "rounds": sl["rounds"],
                                     "games_finished": sl["games_finished"], "tree_resets": sl.get("tree_resets"),
                                     "source": os.path.relpath(longs[-1], ROOT)}
    return out


def pmc_traffic():
    """HBM bytes per round of the tree kernels from the committed PMC passes (profiles/, separate rocprofv3 --pmc runs)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_search_round.json")))
    if not files:
        return None, None
    d = _load_profile(files[-1]) or {}
    return d.get("traffic_bytes_per_launch"), os.path.relpath(files[-1], ROOT)


def library_gemm_peak():
    """what hipBLASLt sustains on an 8192^3 bf16 GEMM on this hardware (tools/gemm_peak.py -> profiles/): the practical
    matrix-pipe ceiling the kernel's issued_bf16_tflops can be read against; the contract's `peak` stays the nominal one"""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_gemm_peak.json")))
    if not files:
        return None
    d = _load_profile(files[-1])
    if not d or not d.get("runs"):
        return None
    return {"value": max(r["tflops"] for r in d["runs"]), "source": os.path.relpath(files[-1], ROOT)}


def pmc_nn(kernel):
    """MFMA utilisation / HBM bytes per launch of a network kernel from the committed PMC passes (profiles/)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_nn.json")))
    if not files:
        return {}
    d = (_load_profile(files[-1]) or {}).get("kernels", {}).get(kernel, {})
    return {"hbm_bytes_per_launch": d.get("hbm_bytes_per_launch"), "mfma_util": d.get("mfma_util"),
            "source": os.path.relpath(files[-1], ROOT)}


def tower_launch_plan(net):
    """What one forward of `net` launches for its residual tower (agent/model.py tower_plan, as executed): a list of
    {step, kernel, blocks, kind, exit}; `kernel` is the key tools/summarize_profiles.py gives that launch's counters.  None when
    the tower does not run as chains."""
    plan = getattr(net, "last_plan", None)
    if not plan or not getattr(net, "chain_blocks", False):
        return None
    kinds = net.block_kinds()
    od = "bf16" if net.operand_dtype == torch.bfloat16 else "f16"
    out = []
    for st in plan:
        if st[0] == "first":
            k = kinds[0]
            kern = {"c6": "k_resblock_c8<FIRST, C6>", "c8": "k_resblock_c8<FIRST>"}.get(k, f"k_resblock_pipe<{od}, FIRST>")
            out.append({"step": "first", "kernel": kern, "blocks": 1, "kind": k, "exit": kinds[1] if len(kinds) > 1 else None})
        elif st[0] in ("tower", "tower_first"):
            k = kinds[st[1][0]]
            first = ", FIRST" if st[0] == "tower_first" else ""
            # (round 6: cz_tower runs on the four-wave pair kernel unless CZ_TOWER4=0; its exits are run-time arguments)
            kern = (f"k_tower<{'HEADS' if st[2] == 'heads' else 'image'}, {k}{first}>" if os.environ.get("CZ_TOWER4", "1")[:1] == "0"
                    else f"k_resblock_ip4_c8<128, {k}>")
            out.append({"step": st[0], "kernel": kern, "blocks": len(st[1]), "kind": k, "exit": st[2]})
        elif st[0] == "pairs":
            out.append({"step": "pairs", "kernel": f"k_tower_pairs<{od}, {'HEADS' if st[2] else 'pairs'}>", "blocks": len(st[1]),
                        "kind": "pair", "exit": "heads" if st[2] else "pair"})
        else:
            k = kinds[st[1]]
            kern = {"c6": "k_resblock_c8<HEADS, C6>", "c8": "k_resblock_c8<HEADS>"}.get(k, "k_resblock")
            out.append({"step": "block", "kernel": kern, "blocks": 1, "kind": k, "exit": "heads"})
    return out


def pmc_tower(arith):
    """HBM bytes per forward of the tower's launches from the committed PMC passes (profiles/rNN_pmc_nn.json, tower_traffic),
    only when that pass profiled the same tower arithmetic."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_nn.json")))
    if not files:
        return {}
    t = ((_load_profile(files[-1]) or {}).get("tower_traffic") or {}).get("per_forward") or {}
    if not t.get("measured_bytes") or t.get("tower_arithmetic") != arith:
        return {}
    return {"hbm_bytes_per_forward": t["measured_bytes"], "algorithmic_activation_bytes_per_forward": t["algorithmic_activation_bytes"],
            "blocks": t["blocks"], "source": os.path.relpath(files[-1], ROOT)}


def arith_label(name):
    """dtype label of a tower arithmetic name (agent/model.py InferenceNet.arith_name)."""
    if name is None:
        return None
    if name.startswith("c8>"):
        return f"f16+2xfp8corr-split(first {name[3:]} blocks)/f16x3-split/f32acc"
    if name.startswith("c6>"):
        return f"f16+2xbf6corr-split(first {name[3:]} blocks)/f16+2xfp8corr-split/f32acc"
    return {"c6": "f16+2xbf6corr-split/f32acc", "c8": "f16+2xfp8corr-split/f32acc", "f16x3": "f16x3-split/f32acc",
            "bf16x3": "bf16x3-split/f32acc", "fp32-library": "f32"}[name]


def arith_mfma_equivalents(name, n_blocks):
    """matrix-pipe time per product in bf16-MFMA units: c8 = one fp16 MFMA + two fp8 MFMAs at twice the rate = 2.0, the
    three-MFMA pairs 3.0, a hybrid tower the mean over its blocks; c6 = one fp16 MFMA + two bf6 MFMAs at four times the rate
    = 1.5 (its first convolution reads the fused input layer's c8 image: 2.0)."""
    if name is None or name == "fp32-library":
        return 1.0
    if name == "c6" or name.startswith("c6>"):      # n6 blocks on c6 (their first convolution of block 0 on c8), the rest on c8
        n6 = int(name[3:]) if name.startswith("c6>") else n_blocks
        return (2.0 + 1.5 * (2 * n6 - 1) + 2.0 * 2 * (n_blocks - n6)) / (2 * n_blocks)
    if name.startswith("c8>"):
        n8 = int(name[3:])
        return (2.0 * n8 + 3.0 * (n_blocks - n8)) / n_blocks
    return {"c8": 2.0, "f16x3": 3.0, "bf16x3": 3.0}[name]


def fp16_tolerance(blocks, filters):
    """Bound for plain fp16 operands (BASELINE configs[4] asks for fp16 MFMA evaluation), derived:
    every convolution output is a sum of 9 F products of operands rounded to fp16 (relative error <= 2^-11 each, so
    <= 2^-10 per product), errors of random sign: relative RMS error of a layer's output ~ 2^-10 / sqrt(3) ~ 6e-4, plus
    2^-11 / sqrt(3) for storing the activation in fp16; the 2 B + 1 layers of the tower add in quadrature (the skip
    connections carry them forward unamplified): e_trunk ~ 7e-4 sqrt(2 B + 1) (B = 20: 4.5e-3).  The heads are
    1-Lipschitz in that relative error times the pre-activation size (|z| <~ 1 for the value, tanh contracts; logits of
    a random-init policy head span <~ 1): value_abs = policy_logit_abs = e_trunk (an upper estimate: the measured worst
    case is 5 x below it), policy_abs = p (1 - p) x logit error <= 1e-4 for p ~ 5e-4."""
    e = 7e-4 * (2 * blocks + 1) ** 0.5
    return {"policy_abs": 1e-4, "value_abs": e, "policy_logit_abs": e,
            "derivation": "fp16 operand rounding 2^-11, random-sign accumulation, quadrature over 2B+1 layers "
                          "(bench.py::fp16_tolerance); measured on the MI355X, 20x256 with perturbed BatchNorm statistics, "
                          "worst of 64 positions: logit 8.4e-4, value 2.3e-4"}


def numerics_check(eng, ref_net, cfg, nq=64):
    """The network the engine ran vs the plain fp32 PyTorch module (CPU) on positions of the last round's queue."""
    qp = eng.queue_planes(nq)           # (rebuilt from the leaves' occupancy boards when the kernel writes only those)
    nq = qp.shape[0]
    with torch.no_grad():
        pg, vg = eng.net(qp)
        pc_, vc_ = ref_net.eval()(qp.float().cpu())
        lg_g, lg_c = torch.log(pg.float().cpu().clamp_min(1e-30)), torch.log(pc_.clamp_min(1e-30))
    lg_g, lg_c = lg_g - lg_g.mean(1, keepdim=True), lg_c - lg_c.mean(1, keepdim=True)   # logits up to a shift
    if cfg.engine.net_dtype == "float32":
        tol = {"policy_abs": 1e-4, "value_abs": 1e-4, "policy_logit_abs": 1e-3}
    elif cfg.engine.net_dtype == "float16":
        tol = fp16_tolerance(cfg.model.res_layer_num, cfg.model.cnn_filter_num)
    else:                                                    # bf16 operands: 2^-8 per operand, 8 x the fp16 bound
        tol = {k: (8 * v if isinstance(v, float) else v)
               for k, v in fp16_tolerance(cfg.model.res_layer_num, cfg.model.cnn_filter_num).items()}
    out = {"positions": nq, "against": "plain PyTorch fp32 module on the CPU, same weights",
           "policy_max_abs_diff": float((pg.float().cpu() - pc_).abs().max()),
           "policy_max_rel_diff": float(((pg.float().cpu() - pc_).abs() / pc_.clamp_min(1e-12)).max()),
           "policy_logit_max_abs_diff": float((lg_g - lg_c).abs().max()),
           "value_max_abs_diff": float((vg.float().cpu() - vc_).abs().max()),
           "tolerance": tol}
    out["within_tolerance"] = bool(out["policy_max_abs_diff"] <= tol["policy_abs"] and
                                   out["value_max_abs_diff"] <= tol["value_abs"] and
                                   out["policy_logit_max_abs_diff"] <= tol["policy_logit_abs"])
    out["primary_figure"] = "policy_logit_max_abs_diff (a random-init policy is ~1/2086 everywhere: absolute policy " \
                            "differences say nothing there; `sharpened` below is the same check on a peaked policy)"
    if cfg.engine.net_dtype == "float32" and getattr(eng, "trunk", None) == "mfma":
        try:
            out["sharpened"] = sharpened_numerics(eng, ref_net, qp)
        except Exception as e:                                # noqa: BLE001
            out["sharpened"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    return out


def sharpened_copy(ref_net, planes, target=0.85):
    """The benchmark's random-init weights with the policy layer scaled until the largest probability on `planes` is
    >= target: the stand-in for a trained (peaked-policy) network -- real cczero weights are not obtainable here
    (.MISSING_LARGE_BLOBS).  Returns (network, scale, float64 outputs on planes)."""
    import copy
    from cchess_alphazero.agent.model import reference_forward_f64
    sharp = copy.deepcopy(ref_net).eval()
    scale, ref = 1.0, None
    for scale in (30.0, 60.0, 120.0, 240.0, 480.0, 960.0):
        sharp.policy_out.weight.data.copy_(ref_net.policy_out.weight.data * scale)
        ref = reference_forward_f64(sharp, planes)
        if float(ref[0].max()) >= target:
            break
    return sharp, scale, ref


def sharpened_numerics(eng, ref_net, planes):
    """north_star's 1e-4 on a PEAKED policy: the benchmark's weights with the policy layer scaled until
    the largest probability on these positions is >= 0.85, evaluated (a) by the arithmetic the engine REQUESTED, unguarded,
    and (b) by what the load-time guard selects for those weights (agent/model.py guarded_inference_net), both against the
    float64 network on the same live-queue positions."""
    from cchess_alphazero.agent.model import guarded_inference_net, measure_against_reference
    sharp, scale, ref = sharpened_copy(ref_net, planes)
    requested = eng.net.arith_requested
    raw = measure_against_reference(guarded_inference_net(sharp, torch.float32, trunk="mfma", arith=requested, guard=False,
                                                          device=planes.device), ref, planes)
    g = guarded_inference_net(sharp, torch.float32, trunk="mfma", arith=requested, device=planes.device)
    m = measure_against_reference(g, ref, planes)
    return {"policy_layer_scale": scale, "max_policy_probability": float(ref[0].max()), "positions": int(planes.shape[0]),
            "against": "float64 evaluation of the same weights on the device (reference_forward_f64)",
            "requested": requested, "requested_unguarded": raw,
            "guard_selected": g.arith_effective, "guard_selected_measured": m,
            "guard_candidates_on_calibration_positions": g.calibration["candidates"] if g.calibration else None,
            "policy_margin": 1e-4 / max(m["policy_max_abs"], 1e-30),
            "within_tolerance": bool(m["policy_max_abs"] <= 1e-4 and m["value_max_abs"] <= 1e-4)}


DUMP_POLICY_ROWS = 1024         # policy rows written by --dump-outputs (2086 float32 each)
DUMP_GAMES = 4096               # games whose root statistics --dump-outputs writes
DUMP_SEED = 20261015            # the fixed sample of rows / games


def _dump_sample(n, k):
    """k indices of range(n), the same for every run with the same n (all of them when n <= k), ascending."""
    import numpy as np
    if n <= k:
        return np.arange(n)
    return np.sort(np.random.RandomState(DUMP_SEED).choice(n, k, replace=False))


def _write_dump(d, arrays, log):
    """arrays: name -> numpy array (float32 / float64 only) -> d/<name>.npy"""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    total = 0
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(d, name + ".npy"), a)
        total += a.nbytes
    assert total <= 64 << 20, f"--dump-outputs: {total} bytes"
    log(f"dumped {len(arrays)} outputs ({total / 2**20:.1f} MiB) to {d}")


def dump_selfplay(d, eng, timed_counters, log):
    """The self-play round's outputs after the last timed step, as a caller of SelfPlayEngine.step receives them:
    the network's evaluation of the leaves the last round queued, by queue SLOT (the compact queue's row order follows the
    kernel's atomics and is not reproducible, its slots are): value of every slot and the policy rows (raw logits where the
    engine runs on logits) of a fixed sample of DUMP_POLICY_ROWS slots, with evaluated = 1 where the slot held a new leaf
    (0 elsewhere, and zeros in value / policy); the search's root statistics of every game (or a fixed sample of DUMP_GAMES
    games) and the counters of the timed leg summed over the ranks (timed_counters: a dict, written in its order -- main's
    `keys`)."""
    import numpy as np
    s = eng.search
    torch.cuda.synchronize()
    out = {}
    row_of_slot = np.arange(s.slots)                   # the queue row that holds a slot's evaluation, -1: none this round
    if eng.compact:
        n = int(s.q_count.item())
        slots = s.q_rows[:n].cpu().numpy().astype(np.int64)
        assert n <= s.slots and (slots >= 0).all() and (slots < s.slots).all()
        row_of_slot = np.full(s.slots, -1, dtype=np.int64)
        row_of_slot[slots] = np.arange(n)
    have = row_of_slot >= 0
    value = s.value.cpu().numpy()[np.maximum(row_of_slot, 0)]
    out["evaluated"] = have.astype(np.float32)
    out["value"] = np.where(have, value, 0.0).astype(np.float32)
    pick = _dump_sample(s.slots, DUMP_POLICY_ROWS)
    rows = torch.from_numpy(np.maximum(row_of_slot[pick], 0)).to(s.policy.device)
    policy = s.policy[rows].cpu().numpy()
    out["policy_slots"] = pick.astype(np.float64)
    out["policy"] = np.where(have[pick][:, None], policy, 0.0).astype(np.float32)
    st = s.root_stats()
    games = _dump_sample(s.G, DUMP_GAMES)
    out["root_games"] = games.astype(np.float64)
    out["root_moves"] = st["moves"][games].astype(np.float64)
    out["root_n"] = st["n"][games].astype(np.float64)
    out["root_w"] = st["w"][games].astype(np.float64)
    out["root_p"] = st["p"][games].astype(np.float32)
    out["root_sum_n"] = st["sum_n"][games].astype(np.float64)
    out["root_counts"] = st["counts"][games].astype(np.float64)
    out["timed_counters"] = np.array([float(v) for v in timed_counters.values()], dtype=np.float64)
    _write_dump(d, out, log)


def run_arena(args, cfg, max_plies=None):
    """BASELINE configs[3]: the evaluator arena on the arena worker (worker/evaluator.py::EvaluateWorker.play_games):
    BestModel vs NextGenerationModel (two random-init networks, seeds 0 / 1), 200 paired games played concurrently,
    two trees per game, 400 simulations per move.  A "step" here is one PLY of the whole arena (every live game makes
    one move: ~sims / K lock-step rounds for the best model's games and as many for the next-generation model's)."""
    from cchess_alphazero import _native
    from cchess_alphazero.agent.model import CChessNet, flops_per_position, guarded_inference_net
    from cchess_alphazero.worker.evaluator import EvaluateWorker, score_table
    dtype = getattr(torch, cfg.engine.net_dtype)
    nets = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        raw = CChessNet.from_model_config(cfg.model)
        model_cfg = raw.cfg
        nets.append(guarded_inference_net(raw, dtype, trunk=cfg.engine.net_trunk,
                                          arith=os.environ.get("CZ_TOWER_ARITH") or cfg.engine.net_arith))
    G = cfg.engine.games_per_gpu
    K = args.sims_per_round or 32
    cfg.opts.evaluate = False                                  # like `run.py eval` of the reference (manager.py:94-103)
    w = EvaluateWorker(cfg, evaluators=tuple(nets), dtype=_native.U8, seed=20260923)
    w.compact = bool(os.environ.get("CZ_ARENA_COMPACT")) and w.compact_capable
    marks = {}

    def on_ply(ply, counters_fn, rounds):
        if ply in (args.warmup, args.warmup + args.steps):
            torch.cuda.synchronize()
            marks[ply] = (time.perf_counter(), counters_fn(), rounds)

    t0 = time.perf_counter()
    stats = {}
    results = w.play_games(G, on_ply=on_ply, stats=stats, sims_per_round=K, stop_after_plies=max_plies)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    a, b = marks[args.warmup], marks.get(args.warmup + args.steps)
    if b is None:
        raise SystemExit("bench.py --config eval: the arena ended before warmup + steps plies")
    dt = b[0] - a[0]
    d = {k: b[1][k] - a[1][k] for k in a[1]}
    rounds = b[2] - a[2]
    table = score_table(results)
    if args.dump_outputs:
        import numpy as np
        # the arena's result as play_games returns it: (value, plies) of every game, in game order
        _write_dump(args.dump_outputs, {"arena_results": np.array(results, dtype=np.float64)},
                    lambda m: print(f"[bench] {m}", file=sys.stderr, flush=True))
    fl = flops_per_position(model_cfg)
    out = {"metric": "mcts_node_expansions_per_sec", "value": d["expansions"] / dt, "unit": "expansions/s", "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None,
           "dtype": arith_label(nets[0].arith_effective) + "+f64/i32 tree",
           "net_arith_requested": nets[0].arith_requested, "net_arith_effective": [n_.arith_effective for n_ in nets],
           "data": "synthetic",
           "config": {"workload": f"BASELINE configs[3] 'eval' ARENA (EvaluateWorker.play_games): {G} paired games "
                                  f"played concurrently, BestModel vs NextGenerationModel = two random-init "
                                  f"{cfg.model.res_layer_num}x{cfg.model.cnn_filter_num} nets (seeds 0 / 1), two trees "
                                  f"per game, {cfg.play.simulation_num_per_move} sims/move, K={K} sims/round/game, "
                                  f"noise_eps {cfg.play.noise_eps}, tau_decay_rate {cfg.play.tau_decay_rate}; "
                                  f"a step = one ply of the whole arena",
                      "games": G, "sims_per_round": K, "parallelism": "one GPU"},
           "sims_per_s": d["sims"] / dt, "rounds_timed": rounds, "ms_per_round": dt / max(1, rounds) * 1e3,
           "queue_rows_per_model_round": G // 2 * K, "compact_queue": bool(w.compact),
           "rows_evaluated_per_round_whole_arena": stats["rows_evaluated"] / max(1, stats["rounds"]),
           "network_tflops": fl * d["expansions"] / dt / 1e12,
           "arena": {"games": G, "plies": stats["plies"], "rounds": stats["rounds"], "seconds": total,
                     "expansions": stats["expansions"], "expansions_per_s_whole_arena": stats["expansions"] / total,
                     "games_per_hour": G / total * 3600.0, "tree_resets": stats["tree_resets"],
                     "overflow_sims": stats["overflow_sims"], "tree_memory": stats["tree_memory"],
                     "score_table": {"next_generation_score": table[0], "games": G,
                                     "red_new_win_draw_fail": list(table[1:4]), "black_new_win_draw_fail": list(table[4:7])},
                     "mean_plies_per_game": sum(t for _, t in results) / len(results),
                     "stopped_after_plies": max_plies}}
    return out


def short_selfplay_leg(label, config, seconds, log, games=None, K=None, dtype=None, trunk=None, model=None, play=None,
                       workload=None, arith=None, sharpen=False):
    """One short self-play leg of another configuration (a few seconds of lock-step rounds from the opening, timed with
    synchronize on both sides; HIP events around the residual-block launches of every round).  sharpen: play with the
    peaked-policy copy of the weights (sharpened_copy) -- the engine's load-time guard then selects the arithmetic such a
    network is allowed, and the leg times THAT."""
    import gc
    from cchess_alphazero.agent.model import CChessNet, events_ms, flops_per_position
    from cchess_alphazero.engine import SelfPlayEngine
    ns = argparse.Namespace(config=config, games=games, sims_per_round=K, dtype=dtype, trunk=trunk)
    cfg = build_config(ns)
    for k, v in (model or {}).items():
        setattr(cfg.model, k, v)
    for k, v in (play or {}).items():
        setattr(cfg.play, k, v)
    t_leg = time.perf_counter()
    torch.manual_seed(0)
    ref_net = CChessNet.from_model_config(cfg.model)
    sharp_rec = None
    if sharpen:
        from cchess_alphazero.agent.model import calibration_planes
        ref_net, scale, ref = sharpened_copy(ref_net, calibration_planes(64, cfg.model.input_depth))
        sharp_rec = {"policy_layer_scale": scale, "max_policy_probability": float(ref[0].max())}
        del ref
    G = cfg.engine.games_per_gpu
    prev_arith = os.environ.get("CZ_TOWER_ARITH")
    if arith:
        os.environ["CZ_TOWER_ARITH"] = arith                  # read by InferenceNet when the engine builds its network
    try:
        eng = SelfPlayEngine(cfg, G, net=ref_net, dtype=getattr(torch, cfg.engine.net_dtype), seed=20260923)
    finally:
        if arith:
            os.environ.pop("CZ_TOWER_ARITH", None)
            if prev_arith is not None:
                os.environ["CZ_TOWER_ARITH"] = prev_arith
    try:
        eng.start(0, 0)
        eng.prewarm()
        for _ in range(3):
            eng.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.step()
        torch.cuda.synchronize()
        est = max(1e-4, time.perf_counter() - t0)
        steps = int(min(400, max(4, seconds / est)))
        keys = ["sims", "expansions", "tree_resets", "overflow_sims", "depth_overflow", "plies"]
        c0 = eng.counters()
        eng.net.block_events = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        c1 = eng.counters()
        d = {k: c1[k] - c0[k] for k in keys}
        blk = events_ms(eng.net.block_events)
        eng.net.block_events = None
        Kq = eng.search.K
        slots = G * Kq
        f, nb = cfg.model.cnn_filter_num, cfg.model.res_layer_num
        split = eng.trunk == "mfma" and cfg.engine.net_dtype == "float32"
        rec = {"workload": workload or f"{G} games/GPU, {cfg.play.simulation_num_per_move} sims/move, K={Kq}, {nb}x{f} net "
                                       f"({cfg.engine.net_dtype}, trunk={eng.trunk}), random-init weights, from INIT_STATE",
               "dtype": (arith_label(eng.net_arith_effective)
                         if split else {"float32": "f32", "bfloat16": "bf16", "float16": "f16"}[
                   cfg.engine.net_dtype]) + "+f64/i32 tree",
               "net_arith_requested": eng.net.arith_requested if split else None,
               "net_arith_effective": eng.net_arith_effective if split else None,
               "value": d["expansions"] / dt, "unit": "expansions/s", "steps": steps, "ms_per_step": dt / steps * 1e3,
               "sims_per_s": d["sims"] / dt, "queue_slots": slots, "compact_queue": bool(eng.compact),
               "policy_rows": "logits" if eng.policy_logits else "softmax",
               "queue_utilisation": d["expansions"] / max(1, steps * slots),
               "tree_resets": d["tree_resets"], "overflow_sims": d["overflow_sims"], "depth_overflow": d["depth_overflow"],
               "tree_gib": eng.search.device_bytes() / 2 ** 30}
        if sharp_rec is not None:
            cal = eng.net.calibration or {}
            rec["peaked_policy"] = dict(sharp_rec, guard_candidates=cal.get("candidates"),
                                        guard_max_policy_probability=cal.get("max_policy_probability"))
        fl = flops_per_position(eng.model_cfg)
        if blk:
            b_ms = sum(blk) / len(blk)
            # boards a launch actually processes: the compact queue's rows (= new leaves), else every slot
            rows_launch = d["expansions"] / steps if eng.compact else slots
            flops_launch = 2 * 2.0 * 90 * f * f * 9 * rows_launch
            tfl = flops_launch / (b_ms * 1e-3) / 1e12
            rec["roofline"] = {"kernel": "residual block (k_resblock family, one launch per block)", "bound": "mfma",
                               "achieved": tfl, "peak": 2500.0, "unit": "TFLOP/s", "frac": tfl / 2500.0,
                               "avg_launch_ms": b_ms, "launches_timed": len(blk), "boards_per_launch": rows_launch,
                               "mfmas_per_product": arith_mfma_equivalents(eng.net_arith_effective, nb) if split else 1,
                               "share_of_step": b_ms * len(blk) / steps / (dt / steps * 1e3),
                               "launch_ms_by_block": [sum(blk[i::nb]) / max(1, len(blk[i::nb])) for i in range(nb)],
                               "launch_plan": [list(st[:2]) + [str(st[2])] for st in (getattr(eng.net, "last_plan", None) or [])
                                               if len(st) > 2] or None}
            if getattr(eng.net, "c6", False):
                rec["roofline"]["arithmetic"] = ("one fp16 MFMA (K = 16) per 16 input channels + two block-scaled bf6 MFMAs "
                                                 "(K = 64, 32 cycles) per 64: 1.5 bf16-MFMA-equivalents per product")
            elif getattr(eng.net, "arith", "") == "c8":
                rec["roofline"]["arithmetic"] = ("one fp16 MFMA (K = 16) per 16 input channels + two block-scaled fp8 MFMAs "
                                                 "(K = 64) per 64: 2.0 bf16-MFMA-equivalents of matrix-pipe time per product")
        else:
            peak = 157.3 if cfg.engine.net_dtype == "float32" and not split else 2500.0
            tf = fl * slots / (dt / steps) / 1e12
            rec["roofline"] = {"kernel": "whole step (tree kernels + network forward; per-convolution launches or library "
                                         "convolutions: no single dominant kernel was timed)", "bound": "mfma",
                               "achieved": tf * (3 if split else 1), "peak": peak, "unit": "TFLOP/s",
                               "frac": tf * (3 if split else 1) / peak, "algorithmic_tflops": tf}
        rec["numerics_check"] = numerics_check(eng, ref_net, cfg)
    finally:
        eng.close()
        del eng
        gc.collect()
        torch.cuda.empty_cache()
    rec["leg_seconds"] = time.perf_counter() - t_leg
    log(f"other_configs[{label}]: {rec['value']:.0f} exp/s, {rec['ms_per_step']:.2f} ms/step, {rec['leg_seconds']:.1f}s")
    return rec


def other_configs(args, log):
    """Short legs of the other single-GPU BASELINE configurations, inside the same invocation:
    deep = configs[4], eval = configs[3] (the arena worker), K40 = the reference's own search_threads of the normal
    config (configs/normal.py:36-37), strict fp32 = the normal config on MIOpen fp32 convolutions (no split operands),
    distribute = the reference's deployed 10 x 192 topology with its play parameters (configs/distribute.py:33-51,84-87)."""
    out = {}
    sec = args.other_config_seconds

    def guarded(label, fn):
        try:
            out[label] = fn()
        except Exception as e:                                # noqa: BLE001  (one failing leg must not void the line)
            out[label] = {"error": f"{type(e).__name__}: {e}"[:400]}
            log(f"other_configs[{label}] FAILED: {out[label]['error']}")
        torch.cuda.empty_cache()

    guarded("deep_20x256_fp16_1600sims", lambda: short_selfplay_leg(
        "deep", "deep", sec, log,
        workload="BASELINE configs[4] 'deep': 4096 games, 1600 sims/move, K=8, 20x256 net, fp16 MFMA operands / fp32 "
                 "accumulate, random-init weights, from INIT_STATE"))

    def arena():
        ns = argparse.Namespace(config="eval", games=None, sims_per_round=None, dtype=None, trunk=None, warmup=2, steps=16,
                                dump_outputs=None)
        r = run_arena(ns, build_config(ns), max_plies=ns.warmup + ns.steps + 1)
        keep = ("value", "unit", "steps", "ms_per_step", "dtype", "sims_per_s", "ms_per_round", "rounds_timed",
                "compact_queue", "rows_evaluated_per_round_whole_arena", "network_tflops")
        rec = {k: r[k] for k in keep}
        rec["workload"] = r["config"]["workload"] + f"; timed plies {ns.warmup}..{ns.warmup + ns.steps} of the arena"
        rec["tree_resets"] = r["arena"]["tree_resets"]
        rec["overflow_sims"] = r["arena"]["overflow_sims"]
        log(f"other_configs[eval]: {rec['value']:.0f} exp/s")
        return rec
    guarded("eval_arena_400sims_200games", arena)
    guarded("normal_K40", lambda: short_selfplay_leg("K40", "normal", sec, log, K=40))
    guarded("normal_bf16x3_tower", lambda: short_selfplay_leg(
        "bf16x3", "normal", sec, log, arith="bf16x3",
        workload="BASELINE configs[1] 'normal' (4096 games, 800 sims/move, K=8, 7x128 net) with round 2's tower "
                 "arithmetic: three bf16 MFMAs per product on (hi, lo) bf16 operand pairs (k_resblock_pipe, fused input "
                 "layer), random-init weights, from INIT_STATE"))
    guarded("normal_f16x3_tower", lambda: short_selfplay_leg(
        "f16x3", "normal", sec, log, arith="f16x3",
        workload="BASELINE configs[1] 'normal' (4096 games, 800 sims/move, K=8, 7x128 net) on the arithmetic the load-time "
                 "guard falls back to for peaked policies: three fp16 MFMAs per product on (hi, lo) fp16 operand pairs "
                 "(22 bits per operand; k_resblock_pipe, fused input layer), random-init weights, from INIT_STATE"))
    guarded("normal_peaked_policy", lambda: short_selfplay_leg(
        "peaked", "normal", sec, log, sharpen=True,
        workload="BASELINE configs[1] 'normal' (4096 games, 800 sims/move, K=8, 7x128 net) on a PEAKED-policy network: the "
                 "benchmark's weights with the policy layer scaled until max p >= 0.85 (the stand-in for trained weights), "
                 "tower arithmetic = what the load-time guard selects for those weights; from INIT_STATE"))
    guarded("mini_1game_50sims_2x32", lambda: short_selfplay_leg(
        "mini", "mini", min(sec, 3.0), log,
        workload="BASELINE configs[0] 'mini' (the reference's own CPU-runnable case): 1 game, 50 sims/move, random-init "
                 "2-block x 32-filter net, from INIT_STATE -- one wavefront and a 1-row network batch on a 256-CU chip: a "
                 "latency figure, reported for completeness"))
    guarded("normal_strict_fp32_library_trunk", lambda: short_selfplay_leg("library", "normal", sec, log, trunk="library"))
    guarded("distribute_10x192_K10_cpuct5", lambda: short_selfplay_leg(
        "distribute", "normal", sec, log, K=10, model=dict(cnn_filter_num=192, res_layer_num=10),
        play=dict(c_puct=5, noise_eps=0.2, max_game_length=200)))
    guarded("distribute_10x192_peaked_policy", lambda: short_selfplay_leg(
        "distribute_peaked", "normal", sec, log, K=10, sharpen=True, model=dict(cnn_filter_num=192, res_layer_num=10),
        play=dict(c_puct=5, noise_eps=0.2, max_game_length=200),
        workload="the reference's deployed topology (configs/distribute.py:33-51,84-87: 10 x 192, K = 10, c_puct 5) with the "
                 "peaked-policy stand-in of a trained network: tower arithmetic = what the load-time guard selects for those "
                 "weights (f16x3 at the end of round 6); from INIT_STATE"))
    return out


def main():
    args = parse()
    if getattr(args, "arith", None):
        os.environ["CZ_TOWER_ARITH"] = args.arith
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s)")
    if args.dry_run:
        return dry_run(args, world, rank)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the engine has no CPU path")
    torch.cuda.set_device(local_rank)
    collective = init_collective(world, rank, args)
    dist_on = dist.is_initialized()
    from cchess_alphazero.agent.model import events_ms, flops_per_position
    from cchess_alphazero.engine import SelfPlayEngine, bytes_per_expansion

    t_start = time.perf_counter()
    if args.plain_resblock or os.environ.get("CZ_RESBLOCK_MODE"):
        from cchess_alphazero import _native
        _native.resblock_pipelined(int(os.environ.get("CZ_RESBLOCK_MODE", "0")))
    cfg = build_config(args)
    if args.config == "eval":
        if world > 1:
            raise SystemExit("bench.py --config eval runs on one GPU (BASELINE configs[3])")
        emit(run_arena(args, cfg))
        return
    dtype = getattr(torch, cfg.engine.net_dtype)
    G = cfg.engine.games_per_gpu
    from cchess_alphazero.agent.model import CChessNet
    torch.manual_seed(0)
    ref_net = CChessNet.from_model_config(cfg.model)          # random-init weights of the named architecture
    eng = SelfPlayEngine(cfg, G, net=ref_net, dtype=dtype, seed=20260923)
    eng.start(first_game_id=rank * G, game_id_stride=world * G)
    K = eng.search.K
    split = eng.trunk == "mfma" and cfg.engine.net_dtype == "float32"
    # the arithmetic the network computes in: split = (hi, lo) bf16 operand pairs, 3 MFMAs per product, fp32 accumulate
    # (what the load-time guard left of the request: agent/model.py guarded_inference_net)
    arith = eng.net_arith_effective if split else None
    if arith == "fp32-library":
        split = False
    # c8: fp16 main term + two block-scaled fp8 (e4m3) correction terms per product; f16x3 / bf16x3: three MFMAs per product
    net_label = (arith_label(arith) if split else
                 {"float32": "f32", "bfloat16": "bf16", "float16": "f16"}[cfg.engine.net_dtype])
    mfma_equiv = arith_mfma_equivalents(arith, cfg.model.res_layer_num) if split else 1.0

    def log(msg):
        if rank == 0:
            print(f"[bench +{time.perf_counter() - t_start:.1f}s] {msg}", file=sys.stderr, flush=True)

    # untimed initialisation: MIOpen solver selection / kernel compilation
    log(f"engine ready ({eng.search.device_bytes() / 2**30:.1f} GiB of trees); prewarm forwards (s): "
        + ", ".join(f"{x:.3f}" for x in eng.prewarm()))
    for _ in range(args.warmup):
        eng.step()
    if args.graph:
        eng.capture_graph(warmup=0)
    torch.cuda.synchronize()
    keys = ["sims", "expansions", "terminal_sims", "repetition_sims", "parked", "sum_depth", "edges_visited",
            "leaf_moves", "plies", "games", "tree_resets", "overflow_sims", "depth_overflow", "chunks_taken", "stat_blocks"]

    def run_leg(n_rounds, sample_every):
        """n_rounds rounds bracketed by barrier + synchronize on both sides; HIP events (same stream) around the tree
        kernels and around every residual-block launch of each sampled round.  Returns (seconds = max over ranks,
        counter deltas summed over ranks + the number of ranks reporting, search-round ms, block ms list)."""
        c0 = eng.counters()
        ev, blk_all = [], []
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_rounds):
            if args.graph:
                eng.step()
                continue
            sampled = i % sample_every == 0
            if eng.net is not None:
                eng.net.block_events = [] if sampled else None
            if sampled:
                e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                e[0].record()
                eng._round()
                e[1].record()
                ev.append(e)
            else:
                eng._round()
            eng._forward()
            eng.rounds += 1
            if sampled and eng.net is not None:
                blk_all += eng.net.block_events
        torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        dt_ = time.perf_counter() - t0
        if eng.net is not None:
            eng.net.block_events = None
        c1 = eng.counters()
        delta = torch.tensor([c1[k] - c0[k] for k in keys] + [1], dtype=torch.int64, device="cuda")
        tmax = torch.tensor([dt_], dtype=torch.float64, device="cuda")
        if dist_on:
            dist.all_reduce(delta, op=dist.ReduceOp.SUM)          # the only collective of the path
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dd = dict(zip(keys + ["ranks"], delta.tolist()))
        # every rank's own rate (a straggler must be visible): one more all-reduce(SUM) of a vector in which a rank fills only
        # its own slot -- still nothing but counter all-reduces on the path
        mine = torch.zeros(world, dtype=torch.float64, device="cuda")
        mine[rank] = (c1["expansions"] - c0["expansions"]) / dt_
        if dist_on:
            dist.all_reduce(mine, op=dist.ReduceOp.SUM)
        dd["per_rank_value"] = mine.tolist()
        k_all = sorted(x.elapsed_time(y) for x, y in ev)
        k_ms_ = sum(k_all) / len(k_all) if ev else None
        dd["search_round_ms_median"] = k_all[len(k_all) // 2] if ev else None
        dd["search_round_ms_max"] = k_all[-1] if ev else None
        b_ms_ = events_ms(blk_all)
        return float(tmax.item()), dd, k_ms_, b_ms_

    dt, d, k_ms, blk_ms = run_leg(args.steps, 1)
    log(f"timed {args.steps} steps in {dt:.2f}s")
    if args.dump_outputs and rank == 0:
        dump_selfplay(args.dump_outputs, eng, {k: d[k] for k in keys}, log)
    extra = extra_legs(args, world)
    n_sus = extra["sustained_rounds"]
    sus = None
    mem_timed = eng.search.memory_info()
    if n_sus > 0:
        eng.drain(1 << 16)                                   # (records of the games that ended so far)
        sus = run_leg(n_sus, 10)
        log(f"sustained leg: {n_sus} rounds in {sus[0]:.1f}s")
        sus_games = eng.drain(1 << 16)                       # rank 0's finished games of the leg (ring: 2 G + 64 records)

    if rank == 0:
        exp_per_launch = d["expansions"] / max(1, args.steps * world)
        mean_d = d["sum_depth"] / max(1, d["sims"])
        mean_c = d["edges_visited"] / max(1, d["sum_depth"])
        mean_l = d["leaf_moves"] / max(1, d["expansions"])
        bpe = bytes_per_expansion(mean_d, mean_c, mean_l)
        slots = G * K
        fl = flops_per_position(eng.model_cfg)
        step_ms = dt / args.steps * 1e3
        out = {
            "metric": "mcts_node_expansions_per_sec", "value": d["expansions"] / dt, "unit": "expansions/s",
            "n_gpus": d["ranks"], "per_rank_value": d["per_rank_value"], "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": step_ms,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": net_label + "+f64/i32 tree",
            "dtype_note": ({"c6": "tower products = f16(w) f16(x) + bf6(w) bf6(x - f16(x)) + bf6(w - f16(w)) bf6(x) (bf6 = e3m2 with a "
                                  "power-of-two scale per tensor from the load-time calibration), fp32 accumulate: ~2^-15 per "
                                  "product (c8, the same sum with e4m3 corrections: 2^-16; bf16x3: 2^-17), fp32-class results -- "
                                  "numerics_check in this line compares the network that just ran with the plain fp32 PyTorch "
                                  "module (north_star tolerance 1e-4 on policy / value); the request is kept only where the "
                                  "load-time check against float64 allows (net_arith_guard); strict fp32: "
                                  "other_configs.normal_strict_fp32_library_trunk",
                            "c8": "tower products = f16(w) f16(x) + e4m3(w) e4m3(x - f16(x)) + e4m3(w - f16(w)) e4m3(x), fp32 "
                                  "accumulate: 2^-16 per product like the split-bf16 form (three bf16 MFMAs per product, "
                                  "other_configs.normal_bf16x3_tower), fp32-class results -- numerics_check in this line "
                                  "compares the network that just ran with the plain fp32 PyTorch module (north_star "
                                  "tolerance 1e-4 on policy / value); strict fp32: other_configs.normal_strict_fp32_library_trunk",
                            "bf16x3": "tower products = three bf16 MFMAs on (hi, lo) bf16 operand pairs, fp32 accumulate: "
                                      "2^-17 per product, fp32-class results (numerics_check in this line)",
                            "f16x3": "tower products = three fp16 MFMAs on (hi, lo) fp16 operand pairs (22 bits per operand), "
                                     "fp32 accumulate, fp32-class results (numerics_check in this line)"}.get(arith)
                           if split else None),
            "net_arith_requested": eng.net.arith_requested if eng.net is not None else None,
            "net_arith_effective": arith,
            "net_arith_guard": (None if eng.net is None or eng.net.calibration is None else
                                {"tol": eng.net.calibration["tol"], "positions": eng.net.calibration["positions"],
                                 "candidates": eng.net.calibration["candidates"],
                                 "tower_activation_max": max(eng.net.calibration["activation_max"]),
                                 "act_shift": eng.net.calibration["act_shift"],
                                 "c8_saturating_layers": eng.net.calibration["c8_saturating_layers"],
                                 "c8_median_in_subnormals": eng.net.calibration["c8_median_in_subnormals"],
                                 "activation_quantiles_scaled_1pct_50pct": eng.net.calibration["activation_quantiles_scaled"]}),
            "data": "synthetic",
            "config": {"workload": f"BASELINE configs[{dict(mini=0, normal=1, eval=3, deep=4)[args.config]}] "
                                   f"'{args.config}': {G} concurrent games/GPU, "
                                   f"{cfg.play.simulation_num_per_move} sims/move, K={K} sims/round/game, "
                                   f"{cfg.model.res_layer_num}x{cfg.model.cnn_filter_num} net "
                                   f"({cfg.engine.net_dtype}, trunk={eng.trunk}), random-init weights, self-play from "
                                   f"INIT_STATE",
                       "games_per_gpu": G, "sims_per_round": K, "queue_slots_per_gpu": slots,
                       "compact_queue": bool(eng.compact),
                       "policy_rows": "logits" if eng.policy_logits else "softmax",
                       "parallelism": f"games sharded over {world} rank(s), no data-path collective"},
            "sims_per_s": d["sims"] / dt, "plies_per_s": d["plies"] / dt,
            "games_per_hour_est": games_per_hour_estimate(d["expansions"] / dt, args.config),
            "queue_utilisation": d["expansions"] / max(1, args.steps * world * slots),
            "games_finished": d["games"],
            "tree_shape": {"mean_depth": mean_d, "mean_edges": mean_c, "mean_leaf_moves": mean_l,
                           "terminal_sims": d["terminal_sims"], "repetition_sims": d["repetition_sims"],
                           "parked": d["parked"], "tree_resets": d["tree_resets"],
                           "chunks_taken": d["chunks_taken"], "stat_blocks": d["stat_blocks"],
                           "overflow_sims": d["overflow_sims"], "depth_overflow": d["depth_overflow"]},
            "tree_memory": dict(mem_timed, when="after the timed steps", chunk_bytes=1 << 20),
            "roofline": None, "roofline_search": None, "roofline_nn": None, "cpu_baseline": None,
        }
        if k_ms is not None:
            ach = bpe * exp_per_launch / (k_ms * 1e-3) / 1e9
            traffic, traffic_src = pmc_traffic()
            out["roofline_search"] = {"kernel": "cz_search_round = k_sim(BACKUP) + k_advance + k_sim(SELECT) (+ k_noise x2)", "bound": "hbm", "achieved": ach, "peak": 8000.0, "unit": "GB/s",
                               "frac": ach / 8000.0, "traffic": traffic, "traffic_source": traffic_src,
                               "algorithmic_bytes_per_launch": bpe * exp_per_launch, "avg_launch_ms": k_ms,
                               "median_launch_ms": d["search_round_ms_median"], "max_launch_ms": d["search_round_ms_max"],
                               "bytes_per_expansion": bpe, "expansions_per_launch": exp_per_launch,
                               "note": "latency / instruction-issue bound pointer chasing (SURVEY 8d), not bandwidth-bound; the algorithmic "
                                       "figure is SURVEY 8(d)'s canonical fp32 accounting (5040-byte planes, whole 8344-byte "
                                       "policy row per expansion) -- the engine writes u8 planes (1260 B) and reads only the "
                                       "legal moves' priors, so the measured PMC traffic is BELOW it"}
            nn_ms = step_ms - k_ms
            tf = fl * slots / (nn_ms * 1e-3) / 1e12
            if split:
                # a product costs mfma_equiv bf16-MFMA units of matrix-pipe time: price that against the dense bf16 peak
                out["roofline_nn"] = {"kernel": f"ResNet forward (hand-written kernels end to end, tower arithmetic {arith})",
                                      "bound": "mfma", "achieved": mfma_equiv * tf, "peak": 2500.0, "unit": "TFLOP/s",
                                      "frac": mfma_equiv * tf / 2500.0, "algorithmic_tflops": tf, "ms": nn_ms,
                                      "positions_per_forward": slots, "mfma_equivalents_per_product": mfma_equiv}
            else:
                peak = 157.3 if cfg.engine.net_dtype == "float32" else 2500.0
                out["roofline_nn"] = {"kernel": "ResNet forward (" + ("k_conv3x3 trunk + " if eng.trunk == "mfma"
                                                                      else "") + "MIOpen/hipBLASLt)",
                                      "bound": "mfma", "achieved": tf, "peak": peak, "unit": "TFLOP/s",
                                      "frac": tf / peak, "ms": nn_ms, "positions_per_forward": slots}
        blk = blk_ms
        if blk:
            # the dominant kernel: k_resblock (one residual block of the tower per launch), > 90 % of a round
            b_ms = sum(blk) / len(blk)
            f = cfg.model.cnn_filter_num
            # two 3x3 convolutions, 2 flop per MAC, on the boards a launch actually processes: the compact queue's
            # rows (= the new leaves of the round), every slot otherwise
            rows_launch = exp_per_launch if eng.compact else slots
            flops_launch = 2 * 2.0 * 90 * f * f * 9 * rows_launch
            tfl = flops_launch / (b_ms * 1e-3) / 1e12
            lplan = tower_launch_plan(eng.net)
            nb_ = cfg.model.res_layer_num
            pmc, pt = {}, pmc_tower(arith)
            if pt:
                # the committed PMC pass of this arithmetic: HBM bytes of a forward's tower launches, per block of the tower
                pmc = {"hbm_bytes_per_launch": pt["hbm_bytes_per_forward"] / pt["blocks"], "source": pt["source"],
                       "algorithmic_activation_bytes_per_block": pt["algorithmic_activation_bytes_per_forward"] / pt["blocks"]}
                mu = [pmc_nn(st["kernel"]).get("mfma_util") for st in (lplan or []) if st["step"] in ("tower", "tower_first", "pairs")]
                pmc["mfma_util"] = next((m for m in mu if m), None)
            arith_text = {"c6": "one fp16 MFMA term + two block-scaled bf6 (e3m2, K = 64, 32 cycles) correction terms",
                          "c8": "one fp16 MFMA term + two block-scaled fp8 (e4m3, K = 64) correction terms",
                          "pair": "three fp16 / bf16 MFMAs on (hi, lo) operand pairs"}
            if lplan:
                kshort = " + ".join(f"{st['kernel']}" + (f" x{st['blocks']} blocks" if st["blocks"] > 1 else "") for st in lplan) + "; per block"
                kinds_used = []
                for st in lplan:
                    if st["kind"] not in kinds_used:
                        kinds_used.append(st["kind"])
                kdesc = ("the residual tower (2 x conv3x3 + bias + skip + ReLU per block) as CHAINS of blocks (csrc/xq_tower.hip; K loops "
                         "csrc/xq_c8_kloop.h / pipe_kloop): a workgroup takes a pair of boards through all blocks of a launch with the "
                         "activations staying in LDS; launches of a forward: " + kshort + ".  The first launch also computes the 5x5 "
                         "input layer (fp32 gather by its copy waves; 'FIRST': inside the chain, for the next pair of boards); 'HEADS' "
                         "launches apply the 1x1 head convolutions as their exit.  Products: " + "; ".join(f"{k}: {arith_text[k]}" for k in kinds_used) + ", fp32 accumulate.  All "
                         "times per BLOCK of the tower (a chained launch spread over its blocks), mean over the tower")
            else:
                kshort = {"c8": "k_resblock_c8 (one residual block per launch)", "c6": "k_resblock_c8<C6> (one residual block per launch)"}.get(
                    arith, "k_resblock_pipe / k_resblock_ip (one residual block per launch)")
                kdesc = ("one residual block (2 x conv3x3 + bias + skip + ReLU) of the tower per launch (csrc/xq_conv.hip); the first "
                         "launch also computes the 5x5 input layer where the kernel exists for the shape, the last one the fused head "
                         "convolutions; mean over all launches of the tower")
            out["roofline"] = {"kernel": kdesc, "kernel_short": kshort,
                               "bound": "mfma", "achieved": tfl, "peak": 2500.0, "unit": "TFLOP/s", "frac": tfl / 2500.0,
                               "traffic": pmc.get("hbm_bytes_per_launch"), "traffic_source": pmc.get("source"),
                               "avg_launch_ms": b_ms, "launches_timed": len(blk), "boards_per_launch": rows_launch,
                               # mean per position in the tower (block 0 hosts the fused input layer, the last one the heads)
                               "launch_ms_by_block": [sum(blk[i::cfg.model.res_layer_num]) / max(1, len(blk[i::cfg.model.res_layer_num]))
                                                      for i in range(cfg.model.res_layer_num)],
                               "first_launch_ms": sum(blk[0::cfg.model.res_layer_num]) / max(1, len(blk[0::cfg.model.res_layer_num])),
                               "algorithmic_flops_per_launch": flops_launch, "launch_plan": lplan,
                               "algorithmic_activation_bytes_per_block": pmc.get("algorithmic_activation_bytes_per_block"),
                               "tower_arithmetic": arith, "mfma_equivalents_per_product": mfma_equiv,
                               "issued_bf16_tflops": mfma_equiv * tfl * 96.0 / 90.0,
                               "issued_frac_of_peak": mfma_equiv * tfl * 96.0 / 90.0 / 2500.0,
                               "mfma_util_pmc": pmc.get("mfma_util"),
                               "library_gemm_bf16_tflops": library_gemm_peak(),
                               "share_of_round": b_ms * len(blk) / args.steps / step_ms,
                               "note": "achieved = fp32-class convolution FLOPs (2 per MAC) / launch time; every product "
                                       "occupies the matrix pipes for mfma_equivalents_per_product bf16-MFMA units (c6: one "
                                       "fp16 MFMA + two bf6 MFMAs at four times the rate = 1.5, 1.54 over the tower with the first "
                                       "convolution on c8; c8: one fp16 + two e4m3 MFMAs at twice the rate = 2.0; bf16x3: 3.0) over 96 pixel slots "
                                       "per 90-pixel board, hence issued_bf16_tflops = that x 96/90 x achieved; against the "
                                       "fp32 matrix peak (157.3 TFLOP/s) the same number is > 1; the chip runs this kernel at "
                                       "its 1.4 kW power cap (profiles/r03_clock_power*.json), not the 2.4 GHz the nominal peak "
                                       "assumes: in shader cycles the c8 K loop runs at 88 % of its MFMA floor (15.7 k cycles per "
                                       "13.8 k of matrix work, profiles/r04_c8_kloop_probe.log), the clock it is granted is "
                                       "1.5-1.8 GHz (in-kernel cycle stamps: profiles/r04_rb_stamps.json); c6: 13.0 k cycles per 10.4 k "
                                       "of matrix work, and the filter stream (576 KB per board and convolution through the CU's "
                                       "64 B/clk vector-memory path) as the second limit (profiles/r04_c6_kloop_probe.log, "
                                       "r04_c6_rb_stamps.json, r04_clock_power_c6_vs_c8.json)"}
        else:
            out["roofline"] = out.get("roofline_search")
        if sus is not None:
            # the sustained leg: games in every phase (openings to endgames), finished games replaced by new ones
            sdt, sd, sk_ms, sblk = sus
            s_exp = sd["expansions"] / sdt
            est = out["games_per_hour_est"] or {}
            mean_plies = est.get("mean_plies_per_game")
            srec = {"rounds": n_sus, "seconds": sdt, "value": s_exp, "unit": "expansions/s",
                    "ms_per_step": sdt / n_sus * 1e3, "sims_per_s": sd["sims"] / sdt,
                    "plies_per_s": sd["plies"] / sdt, "games_finished": sd["games"],
                    "games_per_hour_measured": sd["games"] / sdt * 3600.0,
                    "games_per_hour_steady_state": (sd["plies"] / sdt / mean_plies * 3600.0) if mean_plies else None,
                    "queue_utilisation": sd["expansions"] / max(1, n_sus * world * slots),
                    "tree_resets": sd["tree_resets"], "chunks_taken": sd["chunks_taken"], "stat_blocks": sd["stat_blocks"],
                    "overflow_sims": sd["overflow_sims"], "depth_overflow": sd["depth_overflow"],
                    "mean_depth": sd["sum_depth"] / max(1, sd["sims"]),
                    "search_round_ms": sk_ms, "search_round_ms_median": sd["search_round_ms_median"],
                    "search_round_ms_max": sd["search_round_ms_max"],
                    "tree_memory": dict(eng.search.memory_info(), when="end of the sustained leg", chunk_bytes=1 << 20),
                    "finished_games_rank0": {"n": len(sus_games),
                                             "mean_plies": (sum(g["turns"] for g in sus_games) / len(sus_games)) if sus_games else None,
                                             "resigned": sum(bool(g["resigned"]) for g in sus_games),
                                             "red_black_draw": [sum(g["value"] > 0 for g in sus_games),
                                                                sum(g["value"] < 0 for g in sus_games),
                                                                sum(g["value"] == 0 for g in sus_games)]},
                    "note": "games_per_hour_measured counts the games that FINISHED inside this leg (started from the "
                            "opening together, so early on only short games end); games_per_hour_steady_state = "
                            "measured plies/s / mean plies per game of the committed complete-games run"}
            if sblk:
                sb_ms = sum(sblk) / len(sblk)
                f = cfg.model.cnn_filter_num
                srows = sd["expansions"] / max(1, n_sus * world) if eng.compact else slots
                stfl = 2 * 2.0 * 90 * f * f * 9 * srows / (sb_ms * 1e-3) / 1e12
                srec["roofline"] = {"kernel": "k_resblock", "bound": "mfma", "achieved": stfl, "peak": 2500.0,
                                    "unit": "TFLOP/s", "frac": stfl / 2500.0, "avg_launch_ms": sb_ms,
                                    "launches_timed": len(sblk), "boards_per_launch": srows}
            out["sustained"] = srec
            out["value_sustained"] = s_exp
            out["games_per_hour_steady_state"] = srec["games_per_hour_steady_state"]
            out["roofline_frac_sustained"] = srec.get("roofline", {}).get("frac")
            out["quote"] = ("value = the K timed steps the contract asks for (games in the opening phase); "
                            "value_sustained = the 3000-round leg of the same invocation, games in every phase: the figure "
                            "to quote for self-play throughput")
        if extra["numerics_check"]:
            out["numerics_check"] = numerics_check(eng, ref_net, cfg)
            out["numerics_within_tolerance"] = out["numerics_check"]["within_tolerance"]
            out["numerics_logit_max_abs"] = out["numerics_check"]["policy_logit_max_abs_diff"]
            sh = out["numerics_check"].get("sharpened") or {}
            if "guard_selected_measured" in sh:
                out["numerics_peaked_policy_max_abs"] = sh["guard_selected_measured"]["policy_max_abs"]
                out["numerics_peaked_arith"] = sh["guard_selected"]
        out["roofline_frac"] = (out.get("roofline") or {}).get("frac")
        out["collective"] = collective
    eng.close()                                              # every rank; the legs below need the device memory
    del eng
    import gc
    gc.collect()
    torch.cuda.empty_cache()                                 # (the search object sizes its pool from the FREE memory)
    if rank == 0:
        if extra["other_configs"]:
            out["other_configs"] = other_configs(args, log)
        if extra["micro_suite"]:
            out["micro_suite"] = micro_suite()
            log("micro-suite done")
        if extra["cpu_baseline"]:                            # the CPU leg is reported at N = 1 only
            out["cpu_baseline"] = cpu_baseline(cfg, args.cpu_baseline_seconds)
            out["cpu_tree_only_expansions_per_s"] = out["cpu_baseline"]["value"]
            out["cpu_with_network_estimate"] = out["cpu_baseline"]["with_network_estimate"]["value"]
            log("cpu baseline done")
        pk = (out.get("other_configs") or {}).get("normal_peaked_policy") or {}
        if "value" in pk:
            # the trained-network stand-in: same kernels and shapes, the arithmetic the guard allows a peaked policy
            out["value_peaked_policy"] = pk["value"]
            out["numerics_peaked_arith"] = pk.get("net_arith_effective")
            out["roofline_frac_peaked_policy"] = (pk.get("roofline") or {}).get("frac")
        emit(out)
    if dist_on:
        sys.stdout.flush()
        os.dup2(2, 1)                   # (RCCL's tear-down banner must not follow the JSON line on stdout)
        dist.barrier()                  # rank 0 may still be timing the CPU baseline: leave together
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
