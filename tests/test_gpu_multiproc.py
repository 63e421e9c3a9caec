"""-m gpu: the MULTI-PROCESS side of the tile-sharded frame on a box with one GPU.

Real RCCL refuses two ranks on one device, so the N ranks of `python bench.py --gpus N --oversubscribe` (N processes that share
GPU 0) exchange through tests/tools/fake_rccl.c — a test stand-in for the eleven librccl entry points the library resolves with
dlsym (shared-memory messages; asynchronous and stream-ordered, groups defer their operations to the outermost ncclGroupEnd), selected with LPT_RCCL_LIBRARY.  What this covers, for real and not by emulation:
bench.py's launcher and its N>1 control flow (id rendezvous over gloo, one communicator per renderer, the calibrated tile
weight, barriers, max over ranks), and the library's exchange with world > 1 in separate processes — every rank's send size
against rank 0's receive size and staging offset (the stand-in fails on a mismatch), gather and reduce.  The exchanged frame must
be the single-GPU frame bit for bit: the float64 checksum of the last timed frame equals the one-rank run's.  What it does not
cover is RCCL itself."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "1", "--warmup", "1", "--frames-per-step", "3", "--width", "480", "--height", "270", "--texture-size", "64", "--no-cpu-baseline"]
NOXF = ["--no-exchange-forms"]   # the legs that time the other two exchange forms: only the tests that look at them pay for them


@pytest.fixture(scope="module")
def fake_rccl(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fake_rccl") / "libfake_rccl.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "tools", "fake_rccl.c"),
                           "-o", so, "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-Wl,-rpath,/opt/rocm/lib"])
    return so


def test_the_stand_in_is_stream_ordered_and_defers_grouped_operations(fake_rccl, tmp_path):
    """the properties of RCCL an exchange can get wrong (VERDICT r03 #4 iii): operations run in stream order, asynchronously, and an
    operation recorded inside a group bracket is only enqueued by the OUTERMOST ncclGroupEnd — a consumer enqueued inside the bracket
    reads the old data (tests/tools/fake_rccl_order.c: two threads = two ranks on GPU 0)"""
    exe = str(tmp_path / "fake_rccl_order")
    subprocess.check_call(["gcc", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "tools", "fake_rccl_order.c"),
                           "-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-ldl", "-lpthread", "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe, fake_rccl], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", (p.stdout, p.stderr)


def _bench(extra, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


_ONE = {}


def _one():
    """the one-process line every N>1 test compares its frame with: run once per session"""
    if "j" not in _ONE:
        _ONE["j"] = _bench(["--no-extras"])
    return _ONE["j"]


def test_dump_outputs_gives_the_same_frame_for_the_same_arguments_at_any_rank_count(fake_rccl, tmp_path):
    """`--dump-outputs DIR`: rank 0's presented frame of the last timed step as DIR/radiance.npy (float32, 270 x 480 x RGBA).  Same arguments, same
    frame: a second run, here with two ranks exchanging tiles (equal shares), writes the same pixels bit for bit"""
    import numpy as np
    one = _bench(["--no-extras", "--dump-outputs", str(tmp_path / "one")])
    img = np.load(tmp_path / "one" / "radiance.npy")
    assert img.dtype == np.float32 and img.shape == (270, 480, 4) and one["steps"] == 1 and one["ms_per_step"] > 0
    assert np.all(img[..., 3] == 1.0) and np.all(np.isfinite(img)) and float(img[..., :3].mean()) > 0.0
    _bench(["--gpus", "2", "--oversubscribe", "--root-weight", "8", "--exchange", "gather", "--no-extras", "--dump-outputs", str(tmp_path / "two")] + NOXF,
           {"LPT_RCCL_LIBRARY": fake_rccl})
    assert np.array_equal(np.load(tmp_path / "two" / "radiance.npy"), img)


def test_self_started_ranks_exchange_the_single_gpu_frame(fake_rccl):
    one = _one()
    assert one["n_gpus"] == 1 and one["config"]["frame_complete"] is True
    for n, mode in ((2, "gather"), (3, "reduce"), (3, "gather")):
        j = _bench(["--gpus", str(n), "--oversubscribe", "--root-weight", "8", "--exchange", mode, "--no-extras"] + NOXF, {"LPT_RCCL_LIBRARY": fake_rccl})
        assert j["n_gpus"] == n and j["rccl"]["rccl_nranks"] == n and j["rccl"]["mode"] == mode
        assert j["rccl"]["exchange_frame_complete_on_rank0"] is True
        assert len(j["rccl"]["per_rank_rays"]) == n and all(r > 0 for r in j["rccl"]["per_rank_rays"])
        assert j["rccl"]["exchanges_timed"] == 3
        # equal shares, the same number of frames before it: the last timed frame is the single-GPU frame, bit for bit
        assert j["config"]["frame_checksum"] == one["config"]["frame_checksum"]
        assert j["config"]["rays_per_frame"] == one["config"]["rays_per_frame"]


def test_the_drivers_launcher_command_line(fake_rccl):
    """the contract's N>1 form: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...` —
    the ranks come from the launcher's environment (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*), bench.py starts none itself; rank 0 prints the one JSON line"""
    one = _one()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["LPT_RCCL_LIBRARY"] = fake_rccl
    import socket
    with socket.socket() as sk:      # a free port for the rendezvous
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--oversubscribe", "--root-weight", "8", "--exchange", "gather", "--no-extras"] + SMALL
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines            # rank 0 alone prints
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["rccl"]["rccl_nranks"] == 2 and j["rccl"]["exchange_frame_complete_on_rank0"] is True
    assert j["scaling"] == "strong" or j["scaling"] == "weak"
    assert j["config"]["frame_checksum"] == one["config"]["frame_checksum"]


def test_exchange_inside_a_group_bracket_and_the_denoising_modes_across_processes(fake_rccl):
    """(i) every exchange inside lpt_comm_group_begin / _end: the stand-in enqueues grouped operations only at the outermost ncclGroupEnd,
    so a second phase (unpack) enqueued too early would read stale tiles and the checksum would differ.  (ii) BlitMode::Temporal across two
    processes (BASELINE config 5's form): the filter inputs travel after every call, rank 0 filters, its tile weight is calibrated with
    the filter in the frame (VERDICT r03 #4 iv) — the presented frame equals the one-process frame bit for bit."""
    one = _one()
    j = _bench(["--gpus", "2", "--oversubscribe", "--root-weight", "8", "--exchange", "gather", "--group-bracket", "--no-extras"] + NOXF, {"LPT_RCCL_LIBRARY": fake_rccl})
    assert j["rccl"]["exchange_frame_complete_on_rank0"] is True and j["config"]["frame_checksum"] == one["config"]["frame_checksum"]
    t1 = _bench(["--blit-mode", "temporal", "--no-extras", "--no-shard-emulation"])
    for extra in (["--root-weight", "8", "--exchange", "gather"], ["--group-bracket", "--exchange", "gather"], ["--exchange", "reduce"]):
        t2 = _bench(["--gpus", "2", "--oversubscribe", "--blit-mode", "temporal", "--no-extras"] + extra, {"LPT_RCCL_LIBRARY": fake_rccl})
        assert t2["rccl"]["exchange_frame_complete_on_rank0"] is True, extra
        assert t2["config"]["frame_checksum"] == t1["config"]["frame_checksum"], extra
        assert 0 <= t2["rccl"]["tile_weights"][0] <= 8


def test_host_side_gather_across_processes():
    """`--exchange host`: the timed region needs no RCCL at all — the N processes write their owned pixels into ONE frame in POSIX shared memory behind the C ABI
    (lpt_host_frame_create / _attach, lpt_renderer_read_radiance_owned, lpt_host_frame_barrier: shm + hipHostRegister + progress words, no Python in the protocol);
    the frame is the one-process frame bit for bit.  (Without the stand-in the extra RCCL legs of `exchange_forms` fail — real RCCL refuses two ranks on one
    GPU — and are reported as errors: they must not take the line down.)"""
    one = _one()
    for n in (2, 3):
        j = _bench(["--gpus", str(n), "--oversubscribe", "--exchange", "host", "--no-extras"] + (NOXF if n == 3 else []))
        assert j["n_gpus"] == n and j["rccl"] is None and j["host_gather"]["frame_complete_on_rank0"] is True and j["host_gather"]["ranks"] == n
        assert j["config"]["frame_checksum"] == one["config"]["frame_checksum"] and j["config"]["rays_per_frame"] == one["config"]["rays_per_frame"]
        if n == 2:
            assert j["exchange_forms"]["host"]["timed_region"] is True and j["exchange_forms"]["host"]["frame_checksum"] > 0


def test_one_run_times_all_three_exchange_forms(fake_rccl):
    """an N>1 line carries `exchange_forms` {gather, reduce, host} -> {ms_per_frame, Mrays_s, frame_checksum} — the main form from the timed region, the
    other two from 20 frames each in the same processes — with the three checksums equal, whichever form the timed region used; and the per-rank extremes
    of every stage time (load imbalance of the interleaved tiles)"""
    for main in ("gather", "host", "reduce"):
        j = _bench(["--gpus", "2", "--oversubscribe", "--root-weight", "8", "--exchange", main, "--no-extras"], {"LPT_RCCL_LIBRARY": fake_rccl})
        ef = j["exchange_forms"]
        assert ef["checksums_equal"] is True, ef
        for form in ("gather", "reduce", "host"):
            assert "error" not in ef[form], (main, form, ef[form])
            assert ef[form]["ms_per_frame"] > 0 and ef[form]["Mrays_s"] > 0 and ef[form]["frame_checksum"] == ef[main]["frame_checksum"]
            assert ef[form]["timed_region"] is (form == main)
        sr = j["stage_ms_per_rank"]
        assert "shading" in sr or "path" in sr
        assert all(v["max"] >= v["min"] >= 0.0 and 0 <= v["rank_of_max"] < 2 for v in sr.values())


def test_calibrated_tile_weight_latency_and_frames_in_flight_over_several_communicators(fake_rccl):
    j = _bench(["--gpus", "2", "--oversubscribe", "--exchange", "gather", "--throughput", "--pipeline", "2"] + NOXF, {"LPT_RCCL_LIBRARY": fake_rccl})
    r = j["rccl"]
    assert r["rccl_nranks"] == 2 and r["communicators_per_rank"] == 3 and r["exchange_frame_complete_on_rank0"] is True
    assert len(r["tile_weights"]) == 2 and 1 <= r["tile_weights"][0] <= 8 and r["tile_weights"][1] in (1, 8)
    assert r["tile_weight_calibration"]["rank0_extra_ms"] >= 0.0
    assert j["throughput"]["communicators"] == 2 and j["throughput"]["value"] > 0 and j["latency_ms"]["median"] > 0
    # a forced weight: rank 0 traces 3/11 of the tiles
    k = _bench(["--gpus", "2", "--oversubscribe", "--exchange", "gather", "--root-weight", "3", "--no-extras"] + NOXF, {"LPT_RCCL_LIBRARY": fake_rccl})
    assert k["rccl"]["tile_weights"] == [3, 8] and k["rccl"]["exchange_frame_complete_on_rank0"] is True
    a, b = k["rccl"]["per_rank_rays"]
    assert 0.2 < a / (a + b) < 0.35


def test_a_missing_rccl_library_is_a_loud_error():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["LPT_RCCL_LIBRARY"] = "/nonexistent/librccl.so"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + ["--force-dist", "--exchange", "gather", "--no-extras"], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode != 0 and "librccl could not be loaded" in (p.stderr + p.stdout)      # an RCCL form asked for by name: loud
    # --exchange auto (the default) goes on without it and says why
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + ["--force-dist", "--no-extras", "--no-exchange-forms"], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    j = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert "librccl could not be loaded" in j["rccl"]["error"] and j["config"]["frame_complete"] is True


def test_exchange_auto_picks_the_fastest_form_that_came_up(fake_rccl):
    """`--exchange auto` (the default for N > 1): RCCL comes up under a watchdog, every form gets calibration frames, the timed region uses the
    fastest — and the line says which, with all three forms still reported and their checksums equal"""
    one = _one()
    j = _bench(["--gpus", "2", "--oversubscribe", "--root-weight", "8", "--no-extras"], {"LPT_RCCL_LIBRARY": fake_rccl})     # no --exchange: auto
    ea = j["exchange_auto"]
    assert set(ea["calibration_ms_per_frame"]) == {"host", "gather", "reduce"} and not ea["errors"], ea
    assert ea["chosen"] == min(ea["calibration_ms_per_frame"], key=ea["calibration_ms_per_frame"].get)
    assert j["config"]["exchange"].startswith(ea["chosen"]) and "auto" in j["config"]["exchange"]
    assert j["config"]["frame_complete"] is True and j["config"]["rays_per_frame"] == one["config"]["rays_per_frame"]
    ef = j["exchange_forms"]
    assert ef["checksums_equal"] is True and all("error" not in ef[f] for f in ("gather", "reduce", "host")), ef
    assert ef[ea["chosen"]]["timed_region"] is True
    assert (j["rccl"] is None) == (ea["chosen"] == "host") or "error" not in (j["rccl"] or {})


def test_exchange_auto_survives_an_rccl_bring_up_that_never_returns(fake_rccl):
    """the stand-in's ncclCommInitRank blocks forever (FAKE_RCCL_HANG_INIT): after the watchdog's time (60 s by default, 8 here) the run continues RCCL-free — the line appears, its frame is
    the one-process frame, `config.exchange` says host, `rccl.error` says why, the RCCL forms are reported as errors; the stuck thread is abandoned, nothing is
    restarted and the process leaves with status 0"""
    one = _one()
    j = _bench(["--gpus", "2", "--oversubscribe", "--no-extras", "--rccl-timeout", "8"], {"LPT_RCCL_LIBRARY": fake_rccl, "FAKE_RCCL_HANG_INIT": "1"})
    assert j["n_gpus"] == 2 and j["config"]["exchange"].startswith("host")
    assert "ncclCommInitRank did not return" in j["rccl"]["error"]
    assert j["host_gather"]["frame_complete_on_rank0"] is True
    assert j["config"]["frame_checksum"] == one["config"]["frame_checksum"] and j["config"]["rays_per_frame"] == one["config"]["rays_per_frame"]
    ef = j["exchange_forms"]
    assert ef["host"]["timed_region"] is True and "error" in ef["gather"] and "error" in ef["reduce"]


def test_bench_renders_a_supplied_gltf_with_the_same_span():
    """`bench.py --gltf PATH` (the reference's own assets — DamagedHelmet.glb, sponza3.glb, uffizi-large.hdr — are not in its tree; the Cornell box is):
    the loader's scene instead of the stand-in, the same timed span and line, `data: real`, and the CPU baseline leg reads the same bytes through the oracle's loader"""
    glb = os.path.join(ROOT, "tests", "golden", "cornell-box.glb")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--frames-per-step", "2", "--width", "256", "--height", "256", "--no-extras",
                        "--gltf", glb], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    j = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert j["data"] == "real" and "cornell-box.glb" in j["config"]["workload"] and j["config"]["frame_complete"] is True
    assert 0 < j["accel"]["triangles"] < 100 and j["value"] > 0 and j["config"]["frame_checksum"] > 0
    assert j["cpu_baseline"]["kind"] == "port" and j["cpu_baseline"]["value"] > 0 and "-march=native" in j["cpu_baseline"]["flags"] and j["cpu_baseline"]["threads"] >= 1
