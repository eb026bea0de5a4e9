"""The multi-process GPU scenarios of the suite, run ONCE, BEFORE the first test, from a pytest process that has not
initialised the HIP runtime (tests/conftest.py: pytest_collection_finish); tests/test_z_launch.py - which sorts LAST -
asserts on what they left behind.

Round 4's driver run was red because the two-rank launch test sat at the head of a `-x` suite and hung: 322 parity
tests never ran.  Now a hung or failing launch costs its own deadline (<= 180 s) up front and fails at the END of the
run, after every parity test.  Nothing here is started from a process that has touched the GPU, nothing is exec'ed,
and only the PIDs started here are ever stopped.

Each scenario leaves under <outdir>/<name>/: rank<r>.out / rank<r>.err / rank<r>.phase (deformcontact_amd.launch),
for the bench scenario also launcher.out / launcher.err; RESULTS[name] holds rc, wall time and a failure description.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: name -> {"rc", "wall_s", "timed_out", "dir", "describe", "stdout"}; filled by run_all()
RESULTS = {}
SKIPPED = None          # reason the scenarios were not run (no GPU, HIP already initialised, DC_SKIP_LAUNCH=1)

BENCH_ARGS = ["--gpus", "2", "--steps", "3", "--warmup", "1", "--settle", "0", "--kernel-reps", "4", "--full", "--no-pmc",
              "--no-cpu-baseline", "--no-full-step", "--no-strict-fp32", "--no-radius100k", "--no-merged", "--no-backbones"]
# (NCCL_SOCKET_IFNAME: RCCL bootstraps over sockets even on one node; the loopback interface keeps it off whatever else the
# box has - bench.py sets the same default when the rendezvous address is a loopback one)
DIAG_ENV = {"DC_RANK_WATCHDOG_S": "40", "DC_GLOO_TIMEOUT_S": "60", "NCCL_SOCKET_IFNAME": "lo"}


def _bench_two_rank(out):
    """`python bench.py --gpus 2` (no torchrun): the parent spawns the ranks; two ranks share the box's one device,
    gradient all-reduce over gloo (DC_DIST_BACKEND=gloo exists for exactly this; on the 8-GPU node it is RCCL)."""
    from deformcontact_amd.launch import LaunchResult
    env = dict(os.environ, DC_DIST_BACKEND="gloo", DC_RANK_LOG_DIR=out, DC_LAUNCH_TIMEOUT="170", **DIAG_ENV)
    t0 = time.time()
    with open(os.path.join(out, "launcher.out"), "wb") as fo, open(os.path.join(out, "launcher.err"), "wb") as fe:
        p = subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py")] + BENCH_ARGS, env=env, stdout=fo,
                             stderr=fe, stdin=subprocess.DEVNULL)
        try:
            rc, timed_out = p.wait(timeout=200), False
        except subprocess.TimeoutExpired:                      # (the launcher's own deadline should have fired first)
            p.kill()
            p.wait()
            rc, timed_out = 124, True
    res = LaunchResult(rc, [None, None], timed_out, time.time() - t0, out, 2)
    with open(os.path.join(out, "launcher.out")) as f:
        stdout = f.read()
    with open(os.path.join(out, "launcher.err"), errors="replace") as f:
        err = f.read()[-6000:]
    return {"rc": rc, "timed_out": timed_out, "wall_s": res.wall_s, "dir": out, "stdout": stdout,
            "describe": err, "phases": res.phases()}


def _bench_torchrun(out):
    """The driver's own N > 1 command form - `python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr
    127.0.0.1 --master-port P bench.py --gpus 2 ...` - on the one-device box (gloo, as above): bench.py finds RANK /
    WORLD_SIZE in its environment and is a rank at once; torchrun is the parent and never touches the GPU."""
    from deformcontact_amd.launch import LaunchResult, free_port
    env = dict(os.environ, DC_DIST_BACKEND="gloo", DC_RANK_LOG_DIR=out, **DIAG_ENV)
    for r in range(2):
        try:
            os.remove(os.path.join(out, f"rank{r}.phase"))
        except OSError:
            pass
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "bench.py")] + BENCH_ARGS
    t0 = time.time()
    with open(os.path.join(out, "launcher.out"), "wb") as fo, open(os.path.join(out, "launcher.err"), "wb") as fe:
        p = subprocess.Popen(cmd, env=env, stdout=fo, stderr=fe, stdin=subprocess.DEVNULL, start_new_session=True)
        try:
            rc, timed_out = p.wait(timeout=170), False
        except subprocess.TimeoutExpired:
            import signal
            try:
                os.killpg(p.pid, signal.SIGKILL)               # torchrun's own process group: the agent and its ranks
            except OSError:
                pass
            p.wait()
            rc, timed_out = 124, True
    res = LaunchResult(rc, [None, None], timed_out, time.time() - t0, out, 2)
    with open(os.path.join(out, "launcher.out")) as f:
        stdout = f.read()
    with open(os.path.join(out, "launcher.err"), errors="replace") as f:
        err = f.read()[-6000:]
    return {"rc": rc, "timed_out": timed_out, "wall_s": res.wall_s, "dir": out, "stdout": stdout,
            "describe": err, "phases": res.phases()}


def _bench_rccl_single(out):
    """`DC_BENCH_FORCE_DIST=1 python bench.py` - ONE rank through the N > 1 form of bench.py over RCCL (backend "nccl"):
    process group with `device_id`, parameter broadcast, the captured step replayed with an eager all-reduce + Adam behind
    it, barriers, the float64 MAX of the timing, `all_gather_object` for `dist.ranks_seen`.  Two ranks cannot share the
    box's one device under RCCL; this is as much of the 8-GPU command as one device can run."""
    from deformcontact_amd.launch import launch_ranks
    env = dict(os.environ, DC_BENCH_FORCE_DIST="1", **DIAG_ENV)
    env.pop("DC_DIST_BACKEND", None)
    args = [a if a != "2" else "1" for a in BENCH_ARGS]                       # --gpus 1
    res = launch_ranks(1, [sys.executable, os.path.join(ROOT, "bench.py")] + args, timeout=170, log_dir=out, env=env)
    return {"rc": res.rc, "timed_out": res.timed_out, "wall_s": res.wall_s, "dir": out, "stdout": res.stdout0,
            "describe": res.describe() if res.rc else "", "phases": res.phases()}


def _dp_graphed(branches):
    def run(out):
        from deformcontact_amd.launch import launch_ranks
        env = dict(os.environ, **DIAG_ENV)
        # every GEMM of the step on THIS library's kernels (fixed summation orders): at this size GraphNet would send
        # the attention's q k^T / softmax / p v to stock PyTorch, whose BLAS picks its algorithm per call
        env["DC_FUSED_ATTN"] = "1"
        if branches == "serial":
            env["DC_TEST_SERIAL_BRANCHES"] = "1"
        res = launch_ranks(2, [sys.executable, os.path.join(ROOT, "tests", "dp_graphed_worker.py"),
                               os.path.join(out, "dp")], timeout=150, log_dir=out, env=env)
        return {"rc": res.rc, "timed_out": res.timed_out, "wall_s": res.wall_s, "dir": out, "stdout": res.stdout0,
                "describe": res.describe() if res.rc else "", "phases": res.phases()}
    return run


def _rccl_single(out):
    from deformcontact_amd.launch import launch_ranks
    res = launch_ranks(1, [sys.executable, os.path.join(ROOT, "tests", "rccl_single_worker.py")], timeout=150,
                       log_dir=out, env=dict(os.environ, **DIAG_ENV))
    return {"rc": res.rc, "timed_out": res.timed_out, "wall_s": res.wall_s, "dir": out, "stdout": res.stdout0,
            "describe": res.describe() if res.rc else "", "phases": res.phases()}


SCENARIOS = {"bench_two_rank_gloo": _bench_two_rank, "bench_torchrun_gloo": _bench_torchrun,
             "bench_rccl_single": _bench_rccl_single,
             "dp_graphed_serial": _dp_graphed("serial"),
             "dp_graphed_two_streams": _dp_graphed("two_streams"), "rccl_single": _rccl_single}


def default_outdir():
    return os.environ.get("DC_LAUNCH_OUT", os.path.join(ROOT, "gpurun_out", "launch"))


def _run_one(name, out):
    os.makedirs(out, exist_ok=True)
    t0 = time.time()
    try:
        return SCENARIOS[name](out)
    except Exception as e:                                      # the suite must still run
        return {"rc": 125, "timed_out": False, "wall_s": time.time() - t0, "dir": out, "stdout": "",
                "describe": f"{type(e).__name__}: {e}", "phases": []}


def run_all(names=None, outdir=None):
    """Every scenario once; a failed one ONCE more, from scratch, in a directory of its own (`<name>.attempt2`; the first
    attempt's logs stay where they are).  These are launches of whole processes on a shared box - two ranks time-sharing
    one device over gloo, RCCL bootstrapping over the box's network stack - and round 5 saw each of them stall once on
    boxes where they pass in 4 s a minute later (profiles/r05/t_launch_flakes.txt).  RESULTS[name] is the last attempt,
    with `attempts` and, after a retry, `first_attempt` = the failed one's record.  All of it within DC_LAUNCH_BUDGET_S
    (420 s): once that is spent nothing more is started or retried - the tests that read the missing results fail at the
    END of the run, the parity tests in front of them are not kept waiting."""
    outdir = outdir or default_outdir()
    t_all = time.time()
    budget = float(os.environ.get("DC_LAUNCH_BUDGET_S", "420"))     # all scenarios together, retries included
    for name in (names or SCENARIOS):
        if time.time() - t_all > budget:
            # a box on which launches crawl must not keep the parity tests waiting (round 4: they never ran)
            RESULTS[name] = {"rc": 126, "timed_out": False, "wall_s": 0.0, "dir": os.path.join(outdir, name), "stdout": "",
                             "describe": f"not started: the launch scenarios before it used up their {budget:.0f} s",
                             "phases": [], "attempts": 0}
            continue
        res = _run_one(name, os.path.join(outdir, name))
        res["attempts"] = 1
        if res["rc"] != 0 and os.environ.get("DC_LAUNCH_RETRY", "1") != "0" and time.time() - t_all <= budget:
            first = {k: v for k, v in res.items() if k != "stdout"}
            res = _run_one(name, os.path.join(outdir, name + ".attempt2"))
            res["attempts"], res["first_attempt"] = 2, first
        RESULTS[name] = res
    try:
        with open(os.path.join(outdir, "results.json"), "w") as f:
            json.dump({k: {kk: vv for kk, vv in v.items() if kk != "stdout"} for k, v in RESULTS.items()}, f, indent=1)
    except OSError:
        pass
    return RESULTS


if __name__ == "__main__":                                      # python tests/launch_scenarios.py [name ...] [--loop N]
    sys.path.insert(0, ROOT)
    argv = sys.argv[1:]
    loops = 1
    if "--loop" in argv:
        i = argv.index("--loop")
        loops = int(argv[i + 1])
        del argv[i:i + 2]
    bad = 0
    for it in range(loops):
        r = run_all(argv or None, outdir=os.path.join(default_outdir(), f"loop{it:03d}") if loops > 1 else None)
        for k, v in r.items():
            print(f"[{it}] {k}: rc={v['rc']} timed_out={v['timed_out']} wall={v['wall_s']:.1f}s", flush=True)
            if v["rc"]:
                bad += 1
                print(v["describe"][-4000:], flush=True)
    print(f"{bad} failing scenario runs of {loops * len(argv or SCENARIOS)}")
    sys.exit(1 if bad else 0)
