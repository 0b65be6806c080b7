"""CPU tests of the host side: C-ABI surface, config, LR schedule, sharding, flat arenas, no-fallback."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fovealseg
from fovealseg import hip, ops, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "fovealseg.h")).read()
    return sorted(set(re.findall(r"\b(?:int|long)\s+(fs_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = hip.load()                                  # raises if the .so is missing: no fallback
    declared = _header_symbols()
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/fovealseg.h but not exported"
    assert sorted(list(hip.SIGNATURES) + list(hip.HOST_ONLY)) == declared     # the ctypes table binds exactly the header
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r" T (fs_[a-z0-9_]+)", nm)))
    assert exported == declared


def _header_signatures():
    """{name: (result letter, argument letters)} of every `int|long fs_*( ... );` declaration of the header, in hip.SIGNATURES' letters."""
    src = open(os.path.join(ROOT, "include", "fovealseg.h")).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    letters = {"int": "i", "long": "l", "float": "f", "uint32_t": "u", "unsigned": "u", "fs_stream_t": "p"}
    out = {}
    for res, name, params in re.findall(r"\b(int|long)\s+(fs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        params = [q.strip() for q in params.split(",")]
        if params in (["void"], [""]):
            params = []
        sig = ""
        for q in params:
            words = [t for t in q.replace("*", " * ").split() if t != "const"]
            assert len(words) >= 2, (name, q)                 # a type and a parameter name
            sig += "p" if "*" in words else letters[" ".join(words[:-1])]
        assert name not in out, name
        out[name] = (letters[res], sig)
    return out


def test_ctypes_tables_state_the_headers_parameter_types():
    """Every parameter TYPE of both binding tables against include/fovealseg.h (test_library_exports_every_declared_symbol compares names
    only): a `long` bound as `i` would truncate a scratch size, a float bound as `i` would pass garbage, and either still loads and runs."""
    header = _header_signatures()
    assert sorted(header) == _header_symbols()                 # the parser saw every declaration
    assert len(hip.SIGNATURES) >= 98 and len(hip.HOST_ONLY) >= 43
    for name, sig in hip.SIGNATURES.items():
        assert header[name] == ("i", sig + "p"), (name, header[name], sig)      # hip.load() appends the trailing stream
    for name, entry in hip.HOST_ONLY.items():
        assert header[name] == tuple(entry), (name, header[name], entry)
    # ... and load() binds what the tables say
    lib = hip.load()
    for name, (res, sig) in hip.HOST_ONLY.items():
        fn = getattr(lib, name)
        assert fn.restype is hip._CT[res] and list(fn.argtypes) == [hip._CT[c] for c in sig], name
    for name, sig in hip.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is hip._I and list(fn.argtypes) == [hip._CT[c] for c in sig] + [hip._P], name


def test_stale_library_refuses_to_load(monkeypatch):
    """the library is stamped with a content hash of the sources it was built from, and hip.load() refuses a library whose
    stamp differs from the csrc/ beside it (a shipped .so can never silently be older than its sources)."""
    from fovealseg import build
    assert build.built_hash() == build.source_hash(), "run __graft_entry__.build(): the in-tree library is not built from these sources"
    assert not build.needs_build()
    monkeypatch.setattr(build, "source_hash", lambda flags=build.FLAGS: "0" * 64)
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.delenv("FS_HIP_LIB", raising=False)
    with pytest.raises(hip.HipLibraryError, match="built from other sources"):
        hip.load()


def test_shipped_library_has_no_experiment_switches():
    """Kernel A/B switches exist only in the -DFS_EXPERIMENTS build (csrc/common.h: FS_ENV_INT): the shipped library reads exactly two
    environment variables, FS_CONV_PRECISION and FS_DETERMINISTIC."""
    blob = open(hip.LIB_PATH, "rb").read()
    names = set(re.findall(rb"FS_[A-Z0-9_]{3,}", blob))
    assert names <= {b"FS_CONV_PRECISION", b"FS_DETERMINISTIC"}, sorted(names)
    assert b"FS_CONV_PRECISION" in names and b"FS_DETERMINISTIC" in names


def test_header_is_plain_c(tmp_path):
    """The drop-in boundary is a C ABI: include/fovealseg.h must compile as C99 on its own (no torch, no HIP headers)."""
    src = tmp_path / "t.c"
    src.write_text('#include "fovealseg.h"\nint main(void) { int (*f)(void) = fs_get_conv_precision; return f != 0 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_cpu_fallback():
    with pytest.raises(hip.HipLibraryError):
        hip.ptr(torch.zeros(4))
    with pytest.raises(hip.HipLibraryError):
        ops.gaze_lowres(torch.zeros(1, 3, 8, 8), torch.zeros(1, 2), 4, 4)


def test_cfg_merge_and_defaults():
    cfg = fovealseg.lvis50_cfg()
    assert cfg.MODEL.gaussian_radius == 45 and tuple(cfg.TRAIN.saliency_input_size) == (80, 80)
    cfg.merge_from_list(["TRAIN.task_input_size", "(64,64)", "MODEL.gaussian_radius", "15", "DIR", "x"])
    assert cfg.TRAIN.task_input_size == (64, 64) and cfg.MODEL.gaussian_radius == 15 and cfg.DIR == "x"


def test_builder_errors_match_reference():
    MB = fovealseg.ModelBuilder
    with pytest.raises(Exception, match="Architecture undefined!"):
        MB.build_encoder("resnet50")
    with pytest.raises(Exception, match="Architecture undefined!"):
        MB.build_decoder("upernet")
    sf = MB.build_encoder("segformer", fc_dim=1024)
    assert len(sf.state_dict()) == 1172 and "segformer.encoder.block.2.39.mlp.dwconv.dwconv.weight" in sf.state_dict()
    enc = MB.build_encoder("deeplab", fc_dim=960)
    assert "deeplab.classifier.0.convs.4.1.weight" in enc.state_dict() and len(enc.state_dict()) == 669


def test_state_dict_keys_match_oracle():
    import fovealseg_oracle as O
    m, _ = train.build_module(fovealseg.lvis50_cfg(), device="cpu")
    o = O.OracleDeformSeg()
    sd, so = m.state_dict(), o.state_dict()
    assert set(sd) == set(so) and len(sd) == 2830
    assert all(sd[k].shape == so[k].shape for k in sd)
    # conv weights: reference logical shape, RSCK storage
    w = m.encoder.conv1.weight
    assert tuple(w.shape) == (64, 3, 3, 3) and w.permute(2, 3, 1, 0).is_contiguous()
    # a reference-format checkpoint loads strictly and round-trips
    fovealseg.weights.apply_name_keyed_init(o)
    m.load_state_dict(o.state_dict(), strict=True)
    assert torch.equal(m.state_dict()["encoder.stage3.1.fuse_layers.2.0.0.0.weight"],
                       o.state_dict()["encoder.stage3.1.fuse_layers.2.0.0.0.weight"])


class _Opt:
    def __init__(self, zoom):
        self.param_groups = [dict(lr=2e-5, lr_mult=0.001, zoom=zoom)]


def test_lr_schedule_g12(golden):
    g = golden("g12_lr")
    cfg = fovealseg.lvis50_cfg()
    opts = [_Opt(False), _Opt(False), _Opt(True), _Opt(True)]
    for row in g["table"]:
        train.adjust_learning_rate(opts, 0, cfg, epoch=int(row[0]))
        assert [o.param_groups[0]["lr"] for o in opts] == list(row[1:])


def test_shard_indices_match_distributed_sampler():
    from torch.utils.data.distributed import DistributedSampler
    ds = list(range(103))
    for world in (1, 2, 8):
        seen = []
        for rank in range(world):
            ref = list(DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=True, seed=0))
            got = train.shard_indices(len(ds), rank, world, epoch_seed=0, shuffle=True)
            assert got == ref
            seen += got
        assert set(seen) == set(ds)


def test_flat_params_views_and_strides():
    w = torch.nn.Parameter(ops.new_rsck_weight(8, 4, 3, 3).normal_())
    b = torch.nn.Parameter(torch.randn(5))
    w0, b0 = w.detach().clone(), b.detach().clone()
    fp = train.FlatParams([w, b])
    assert fp.numel % 4 == 0 and torch.equal(w, w0) and torch.equal(b, b0)
    assert w.permute(2, 3, 1, 0).is_contiguous() and w.grad.stride() == w.stride()
    w.grad.add_(1.0)
    assert float(fp.grad.sum()) == w.numel()
    fp.zero_grad()
    assert float(fp.grad.abs().sum()) == 0.0 and w.grad.data_ptr() == fp.grad.data_ptr()
    with torch.no_grad():
        fp.data.mul_(2.0)
    assert torch.equal(w, 2 * w0)


def test_dropout_hash_statistics():
    import fovealseg_oracle as O
    keep = O.dropout_keep_mask_nhwc(1 << 20, ops.layer_key(3, 77), 0.3)
    assert abs(keep.mean() - 0.7) < 2e-3
    assert O.layer_key(3, 77) == ops.layer_key(3, 77)
    assert not np.array_equal(keep, O.dropout_keep_mask_nhwc(1 << 20, ops.layer_key(3, 78), 0.3))


def test_pad_weight_channels_and_fanout_subsample_autograd():
    """Host-side autograd glue added for the odd-channel and strided-shortcut layers (pure tensor logic, no kernel)."""
    import torch
    from fovealseg import ops
    g = torch.Generator().manual_seed(3)
    # PadWeightChannels: zero taps for the padding channels, gradient sliced back to the parameter's shape
    w = ops.new_rsck_weight(6, 5, 3, 3)
    w.copy_(torch.randn(6, 5, 3, 3, generator=g))
    w.requires_grad_(True)
    wp = ops.PadWeightChannels.apply(w, 16)
    assert wp.shape == (6, 16, 3, 3) and ops.rsck(wp).is_contiguous()
    assert torch.equal(wp[:, :5].detach(), w.detach()) and float(wp[:, 5:].detach().abs().max()) == 0.0
    cot = torch.randn(6, 16, 3, 3, generator=g)
    (wp * cot).sum().backward()
    assert torch.equal(w.grad, cot[:, :5])
    assert ops.padded_in_channels(3) == 16 and ops.padded_in_channels(5) == 16 and ops.padded_in_channels(18) == 20
    # FanOutSubsample: forward = (x, x[:, ::s, ::s]); backward adds the subsampled gradient at the sampled pixels
    x = torch.randn(2, 9, 10, 4, generator=g, requires_grad=True)
    xf, xs = ops.FanOutSubsample.apply(x, 4)
    assert torch.equal(xf, x) and torch.equal(xs, x[:, ::4, ::4, :])
    gf, gs = torch.randn(xf.shape, generator=g), torch.randn(xs.shape, generator=g)
    ((xf * 1.0 * gf).sum() + (xs * gs).sum()).backward()
    want = gf.clone()
    want[:, ::4, ::4, :] += gs
    assert torch.allclose(x.grad, want)
    # only the subsampled branch used
    x2 = torch.randn(1, 5, 5, 2, generator=g, requires_grad=True)
    _, xs2 = ops.FanOutSubsample.apply(x2, 2)
    xs2.sum().backward()
    want2 = torch.zeros_like(x2)
    want2[:, ::2, ::2, :] = 1.0
    assert torch.equal(x2.grad, want2)


def test_driver_contract_surface():
    """bench.py takes the driver's flags and __graft_entry__ exposes build() / smoke(); nothing here touches a GPU."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    for flag in ("--gpus", "--steps", "--warmup", "--conv-precision", "--full", "--dump-outputs", "--deterministic"):
        assert flag in out.stdout
    src = open(os.path.join(root, "bench.py")).read()
    for key in ('"metric"', '"value"', '"unit"', '"n_gpus"', '"ms_per_step"', '"higher_is_better"', '"scaling"', '"vs_baseline"', '"dtype"',
                '"data"', '"config"', '"roofline"', '"cpu_baseline"'):
        assert key in src, key
    assert "/root/reference" not in src                      # nothing on the GPU box may read the reference
    sys.path.insert(0, root)
    import __graft_entry__ as g
    assert callable(g.build) and callable(g.smoke)
    entry = open(os.path.join(root, "__graft_entry__.py")).read()
    assert "gfx950" in entry or "build.py" in entry


def test_conv_dispatch_predicate_above_4gb():
    """the channel-aligned kernels address the source with 32-bit BYTE offsets, so a source of 4 GB or more
    (>= 2^30 fp32 elements) must take the 64-bit-indexed generic kernel, never wrap.  Host-side predicate, no launch."""
    from fovealseg import hip
    lib = hip.load()
    saved = lib.fs_get_conv_precision()
    try:
        for mode in (0, 1, 2):
            assert lib.fs_set_conv_precision(mode) == 0
            ws = 1 << 30
            # 1x1 bottleneck conv, B*H*W*256 elements: just below / above 2^30 elements (4 GB)
            below = lib.fs_conv2d_kernel_choice(63, 256, 256, 256, 256, 256, 64, 1, 1, 1, 0, 1, 0, ws)        # 3.94 GB
            above = lib.fs_conv2d_kernel_choice(64, 256, 256, 256, 256, 256, 64, 1, 1, 1, 0, 1, 0, ws)        # 4.00 GB
            assert below == (4 if mode else 1) and above == 0, (mode, below, above)      # 4 = the 1x1 GEMM kernel of the split modes
            # between 4 and 8 GB (2^30..2^31 elements) -- the range the old `elements < 2^31` guard let through
            assert lib.fs_conv2d_kernel_choice(100, 256, 256, 256, 256, 256, 64, 1, 1, 1, 0, 1, 0, ws) == 0
            # 3x3 stride 1: halo kernel (its F(2,3) variant, 5, where the width is even; plain halo, 2, on odd widths) below 4 GB
            # in the split modes, generic above (source or destination)
            small = lib.fs_conv2d_kernel_choice(64, 80, 80, 64, 80, 80, 64, 3, 3, 1, 1, 1, 0, ws)
            wino_on = os.environ.get("FS_WINOGRAD", "1") != "0"
            # (8 = the F(4,3) kernel of round 5: bf16x3, widths that are multiples of 4; 5 = F(2,3))
            assert small == ((8 if wino_on and mode == 1 else 2) if mode else 1), (mode, small)      # f16x2: from 128 channels up
            wide = lib.fs_conv2d_kernel_choice(64, 40, 40, 128, 40, 40, 128, 3, 3, 1, 1, 1, 0, ws)
            assert wide == (((8 if mode == 1 else 5) if wino_on else 2) if mode else 1), (mode, wide)
            # five pairs per row, not whole quads: F(2,3); a wide 20-wide layer: F(4,3) as well (its eight-wave form)
            assert lib.fs_conv2d_kernel_choice(64, 10, 10, 64, 10, 10, 64, 3, 3, 1, 1, 1, 0, ws) == ((5 if wino_on and mode == 1 else 2) if mode else 1)
            assert lib.fs_conv2d_kernel_choice(64, 20, 20, 256, 20, 20, 256, 3, 3, 1, 1, 1, 0, ws) == (((8 if mode == 1 else 5) if wino_on else 2) if mode else 1)
            odd = lib.fs_conv2d_kernel_choice(64, 81, 81, 64, 81, 81, 64, 3, 3, 1, 1, 1, 0, ws)
            assert odd == (2 if mode else 1), (mode, odd)
            assert lib.fs_conv2d_kernel_choice(2800, 80, 80, 64, 80, 80, 64, 3, 3, 1, 1, 1, 0, ws) == 0       # 4.6 GB source
            # stride 2 forward with a source >= 4 GB and a destination < 4 GB: falls back instead of raising
            assert lib.fs_conv2d_kernel_choice(2800, 80, 80, 64, 40, 40, 128, 3, 3, 2, 1, 1, 0, ws) == 0
            # bwd-data: the source is dY
            assert lib.fs_conv2d_kernel_choice(2800, 80, 80, 64, 80, 80, 64, 3, 3, 1, 1, 1, 1, ws) == 0
            # unaligned channels always take the generic kernel
            assert lib.fs_conv2d_kernel_choice(2, 20, 20, 3, 20, 20, 64, 3, 3, 1, 1, 1, 0, ws) == 0
    finally:
        lib.fs_set_conv_precision(saved)


def test_bench_self_launch_command(monkeypatch):
    """`bench.py --gpus N` without a launcher spawns `python -m torch.distributed.run` with N ranks on 127.0.0.1 (VERDICT r1 #6a)."""
    import importlib
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    bench = importlib.import_module("bench")
    seen = {}

    class Done:
        returncode = 0

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return Done()
    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = bench.parse_args()
    assert bench.self_launch(args) == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    # the three modes and the headline rule are part of the line's contract
    assert set(bench.MODES) == {"f32", "bf16x3", "f16x2"} and bench.MODES["bf16x3"][2] == 24
    assert bench.mode_peak("bf16x3") == 2500.0 / 6 and bench.mode_peak("f16x2") == 2500.0 / 3 and bench.mode_peak("f32") == 157.3


def test_bench_line_is_short_and_parseable(tmp_path, monkeypatch):
    """VERDICT r2 #1 / ADVICE r2 (high): the final stdout line must stay under 2 KB whatever the per-kernel tables hold, parse as JSON,
    and carry the headline mode's value, ONE roofline object and cpu_baseline; everything else goes to bench_detail.json."""
    import importlib
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    bench = importlib.import_module("bench")
    # a fake KernelTimer summary with every kind roofline_entries knows, so the per-mode detail is as large as it gets
    kinds = ["conv3x3", "wgrad3x3", "conv_affine", "conv_wgrad", "bn_fwd", "bn_bwd"] + list(bench.FRONTEND_KINDS)
    summ = {k: {"flops": 3.9705e10 * 438 * 20, "total_ms": 71.0 * 20, "launches": 438 * 20} for k in kinds}
    results = {}
    for i, mode in enumerate(("bf16x3", "f16x2", "f32")):
        res = {"value": 331.7 - 10 * i, "unit": "img/s", "ms_per_step": 192.9 + i, "operand_significand_bits": bench.MODES[mode][2],
               "arithmetic": bench.MODES[mode][3], "loss": 1.234}
        res.update(bench.roofline_entries(mode, summ, 20, 4.1))
        results[mode] = res
    fwd_only = {m: {"img_per_s": 1160.5, "ms_per_batch": 55.15, "algorithmic_tflops": 176.7} for m in results}
    cpu = {"value": 1.6754, "unit": "img/s", "cores": 16, "kind": "port", "sample": "x" * 400, "forward_only": {"value": 4.979, "sample": "y" * 200}}
    line, detail = bench.build_lines("bf16x3", 1, 20, 5, 64, 1024, results, fwd_only, cpu)
    text = json.dumps(line)
    assert len(text) < 2048 and "\n" not in text, len(text)
    back = json.loads(text)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "cpu_baseline", "modes"):
        assert key in back, key
    assert back["value"] == 331.7 and back["conv_precision"] == "bf16x3" and back["config"]["workload"].startswith("configs[1]")
    assert "model" not in back["config"]
    r = back["roofline"]
    # round 5: the line says what each number is -- kernel_avg_us (rocprof, the kernels alone) beside avg_launch_us (in-process
    # bracket around the C-ABI call incl. the weight pack), traffic marked as not measured in this run, the share of the products executed
    assert set(r) == {"kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_measured_in_this_run", "launches_per_step",
                      "avg_launch_us", "kernel_avg_us", "executed_mfma_fraction"}
    assert r["traffic_measured_in_this_run"] is False
    assert len(r["kernel"]) <= 80 and r["kernel"].startswith("conv3x3_wino4_kernel<PrecX3>") and r["bound"] == "mfma"
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert set(back["cpu_baseline"]) == {"value", "unit", "cores", "kind", "sample"} and back["cpu_baseline"]["kind"] == "port"
    assert set(back["modes"]) == set(results) and set(back["modes"]["f32"]) == {"value", "ms_per_step", "frac"}
    # the detail keeps what the line dropped, and lands in a side file
    assert "frontend" in detail["modes"]["bf16x3"] and detail["forward_only"] is fwd_only
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    bench.write_detail(detail)
    assert json.load(open(tmp_path / "bench_detail.json"))["line"]["value"] == 331.7
    # a multi-GPU line (no cpu_baseline on N>1) is just as short
    line8, _ = bench.build_lines("bf16x3", 8, 20, 5, 64, 1024, results, None, None)
    assert len(json.dumps(line8)) < 2048 and line8["n_gpus"] == 8 and line8["config"]["global_batch"] == 512
    # nothing is printed after the JSON line
    src = open(os.path.join(root, "bench.py")).read()
    tail = src[src.index("print(json.dumps(line)"):src.index("MAX_LINE_BYTES = 2048")]
    assert "print(" not in tail[len("print(json.dumps(line)"):]


def test_bench_plain_run_times_the_headline_alone(monkeypatch):
    """A plain `bench.py --gpus 1 --steps N --warmup W` times the headline mode only; --full times all three (headline first), --modes
    and --conv-precision still choose explicitly."""
    import importlib
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")

    def modes(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", *argv])
        args = bench.parse_args()
        return bench.run_modes(args), args

    m, args = modes()
    assert m == ["bf16x3"] and not args.full and args.dump_outputs is None and args.steps == 3 and args.warmup == 1
    assert modes("--full")[0] == ["bf16x3", "f16x2", "f32"]
    assert modes("--full", "--headline", "f32")[0] == ["f32", "bf16x3", "f16x2"]
    assert modes("--conv-precision", "f16x2", "--full")[0] == ["f16x2"]
    assert modes("--modes", "f32,bf16x3")[0] == ["bf16x3", "f32"]
    assert modes("--dump-outputs", "out")[1].dump_outputs == "out"


def test_bench_dump_outputs_layout(tmp_path):
    """--dump-outputs writes the step's return values, the arenas' parameters and gradients (a fixed sorted sample of the large ones)
    and the float buffers, all float32, within 64 MB; the sample indices do not depend on the run."""
    import importlib
    import types
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    g = torch.Generator().manual_seed(0)
    sizes = (bench.DUMP_SAMPLE + 1000, 1000, 28)
    datas = [torch.randn(n, generator=g) for n in sizes]
    # grad = 2 * data elementwise: a params / grads pair taken at different indices cannot satisfy grads == 2 * params
    opts = [types.SimpleNamespace(flat=types.SimpleNamespace(numel=n, data=d, grad=2 * d)) for n, d in zip(sizes, datas)]
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 1), torch.nn.BatchNorm2d(4))
    out = (torch.tensor(1.5), torch.tensor(0.25), torch.tensor(0.125, dtype=torch.float64))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, opts, net)
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == sorted(["loss", "acc", "edge_loss", "buffers"] + [f"{k}_{a}" for k in ("params", "grads") for a in bench.ARENA_NAMES[:3]])
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "edge_loss.npy").tolist() == [0.125]
    idx = np.sort(np.random.default_rng(0).choice(sizes[0], bench.DUMP_SAMPLE, replace=False))       # the documented sample: seed 0, sorted
    big = np.load(tmp_path / "a" / "params_encoder.npy")
    assert big.shape == (bench.DUMP_SAMPLE,) and np.array_equal(big, datas[0].numpy()[idx])
    for arena in bench.ARENA_NAMES[:3]:                    # every params / grads pair at the same elements
        assert np.array_equal(np.load(tmp_path / "a" / f"grads_{arena}.npy"), 2 * np.load(tmp_path / "a" / f"params_{arena}.npy")), arena
    assert np.array_equal(np.load(tmp_path / "a" / "grads_decoder.npy"), opts[1].flat.grad.numpy())
    assert np.load(tmp_path / "a" / "buffers.npy").shape == (8,)          # BatchNorm running mean + var (num_batches_tracked is an integer)


@pytest.mark.gpu
def test_bench_plain_run_line_and_dump(tmp_path):
    """Bench runs on the device at a small size.  A plain run times the library's default mode and its line carries the headline figure with
    nothing of --full.  --dump-outputs (implies --deterministic) leaves finite float32 arrays of the LAST timed step: its loss is the line's
    `loss`, a run with one timed step fewer dumps another loss, and two runs with the same arguments write the same arrays bit for bit
    (several steps on one batch would amplify any run-to-run difference of the default mode's atomics)."""
    import json

    def run(name, steps, *extra):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--batch", "2",
               "--size", "256", *extra]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, (name, r.stderr[-3000:])
        line = json.loads(r.stdout.strip().splitlines()[-1])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["steps"] == steps and line["warmup"] == 2 and line["unit"] == "img/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f32" and line["value"] > 0 and abs(line["value"] - 2 * 1000.0 / line["ms_per_step"]) <= 1e-2 * line["value"]
        assert list(line["modes"]) == ["bf16x3"] and "cpu_baseline" not in line and line["roofline"] is None and "detail" not in line
        dump = None
        if os.path.isdir(tmp_path / name):
            dump = {f[:-4]: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))}
        return line, dump

    plain, none = run("plain", 3)
    assert plain["config"]["deterministic"] is False and none is None          # the yardstick: the library's default mode, no dump
    lines, dumps = zip(*(run(n, s, "--dump-outputs", str(tmp_path / n)) for n, s in (("a", 3), ("b", 3), ("c", 2))))
    assert all(l["config"]["deterministic"] is True for l in lines)
    for line, dump in zip(lines, dumps):
        assert dump["loss"].dtype == np.float32 and dump["loss"].shape == (1,) and np.float32(line["loss"]) == dump["loss"][0]
    for name in ("params_encoder", "grads_encoder", "params_decoder", "buffers"):
        a = dumps[0][name]
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), name
    assert set(dumps[0]) == set(dumps[1]) == set(dumps[2])
    for name, a in dumps[0].items():
        assert np.array_equal(a, dumps[1][name]), name
    assert dumps[2]["loss"][0] != dumps[0]["loss"][0] and not np.array_equal(dumps[2]["params_encoder"], dumps[0]["params_encoder"])


# ------------------------------------------------------------------------------------------------
# pins captured from the reference itself (tests/golden/make_pins.py; VERDICT r1 "next" #8)
# ------------------------------------------------------------------------------------------------
def _pin(name):
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as f:
        return json.load(f)


def test_state_dict_matches_reference_key_shape_list():
    """key -> shape -> dtype of the module's state_dict against the list dumped from the REFERENCE module (2 830 entries,
    130 684 598 elements), in the reference's own order: a checkpoint written by either side loads strictly into the other."""
    table = _pin("g15_state_dict.json")
    assert len(table) == 2830
    m, _ = train.build_module(fovealseg.lvis50_cfg(), device="cpu")
    sd = m.state_dict()
    assert [k for k, _, _ in table] == list(sd.keys())                       # same keys, same order
    for k, shape, dtype in table:
        assert list(sd[k].shape) == shape, (k, tuple(sd[k].shape), shape)
        assert str(sd[k].dtype).replace("torch.", "") == dtype, (k, sd[k].dtype, dtype)
    # the oracle holds the same list (it is what the goldens were generated against)
    import fovealseg_oracle as O
    so = O.OracleDeformSeg().state_dict()
    assert {k: list(v.shape) for k, v in so.items()} == {k: s for k, s, _ in table}


def test_lvis50_cfg_matches_reference_effective_config():
    """Every key of lvis50_cfg() against the reference's own config/defaults.py + config/deform.yaml + README.md:79 overlay."""
    ref = _pin("g15_config.json")
    cfg = fovealseg.lvis50_cfg()
    # not configuration of the reference but of this bench / of run-time state: named here, every other key must match
    exempt = {("DIR",),                                           # checkpoint directory name
              ("DATASET", "grid_path"), ("DATASET", "list_train"), ("DATASET", "root_dataset"),      # files (grid PNG is dead code)
              ("TRAIN", "batch_size_per_gpu"),                    # BASELINE configs[1] batch 64 (reference yaml: 1)
              ("TRAIN", "max_iters"), ("TRAIN", "running_lr_encoder"), ("TRAIN", "running_lr_decoder"), ("TRAIN", "running_lr_foveater")}  # set at run time (train_deform_semantic.py:626-629)

    def norm(v):
        return [norm(x) for x in v] if isinstance(v, (tuple, list)) else v
    checked = 0
    for sec, node in cfg.items():
        if not isinstance(node, dict):
            assert (sec,) in exempt
            continue
        for k, v in node.items():
            if (sec, k) in exempt:
                continue
            assert k in ref[sec], f"{sec}.{k} is not a key of the reference configuration"
            assert norm(v) == norm(ref[sec][k]), (sec, k, v, ref[sec][k])
            checked += 1
    assert checked >= 70
    assert ref["TRAIN"]["epoch_iters"] * ref["TRAIN"]["num_epoch"] == cfg.TRAIN.max_iters


def test_train_step_skips_frozen_optimisers(monkeypatch):
    """train_deform_semantic.py:112-120: inside the fix_deform window the zoom optimisers do not step (their Adam state must not
    advance), inside the fix_seg window the segmentation optimisers do not."""
    calls = []

    class Opt:
        def __init__(self, zoom):
            self.param_groups = [dict(lr=1.0, lr_mult=1.0, zoom=zoom)]
            self.zoom = zoom

        def zero_grad(self):
            pass

        def step(self):
            calls.append(self.zoom)

    class Loss:
        def mean(self):
            return self

        def backward(self):
            pass
    monkeypatch.setattr(train, "allreduce_gradients", lambda opts, module=None: None)
    opts = [Opt(False), Opt(False), Opt(True), Opt(True)]
    module = lambda feed, epoch=None, cur_iter=None: (Loss(), None, None)       # noqa: E731
    batch = (torch.zeros(1, 4, 2, 2), None, None, None)
    cfg = fovealseg.lvis50_cfg()
    train.train_step(module, opts, batch, cfg, epoch=1)
    assert calls == [False, False, True, True]
    calls.clear()
    cfg.TRAIN.fix_deform_aft_pretrain, cfg.TRAIN.fix_deform_start_epoch, cfg.TRAIN.fix_deform_end_epoch = True, 3, 5
    train.train_step(module, opts, batch, cfg, epoch=4)
    assert calls == [False, False]
    calls.clear()
    train.train_step(module, opts, batch, cfg, epoch=6)
    assert calls == [False, False, True, True]
    calls.clear()
    cfg.TRAIN.fix_deform_aft_pretrain = False
    cfg.TRAIN.opt_deform_LabelEdge, cfg.TRAIN.fix_seg_start_epoch, cfg.TRAIN.fix_seg_end_epoch = True, 2, 2
    train.train_step(module, opts, batch, cfg, epoch=2)
    assert calls == [True, True]


def test_flat_adam_refuses_gradients_outside_its_arena():
    """a caller following the reference loop (`module.zero_grad()` -> .grad = None -> fresh .grad tensors) must
    not get a silent weight-decay-only step."""
    net = torch.nn.Linear(4, 3)
    opt = train.FlatAdam(list(net.parameters()), lr=1e-3, weight_decay=1e-4, lr_mult=1.0, zoom=False)
    opt.check_grads_in_arena()                                   # fresh arena views: fine
    net.zero_grad(set_to_none=True)
    net(torch.randn(2, 4)).sum().backward()                      # autograd allocates new .grad tensors outside the arena
    with pytest.raises(RuntimeError, match="gradient-arena"):
        opt.check_grads_in_arena()
    want = [p.grad.clone() for p in net.parameters()]
    opt.flat.adopt_grads()
    opt.check_grads_in_arena()
    assert all(torch.equal(p.grad, w) for p, w in zip(net.parameters(), want))
    assert float(opt.flat.grad.abs().sum()) > 0


def test_stash_grad_hands_the_second_reader_gradient_to_the_conv_consumer():
    """ops.StashGrad (C1: `feat` read by the mask branch's conv and by the classification branch) on CPU tensors, with a stand-in for the conv
    consumer that does what ConvBnAct.backward does with the fan-out's records: (a) stash node created AFTER the conv branch in the forward ->
    the engine runs it first, the conv consumer finds the gradient in PENDING_RES and the fan-out adds nothing; (b) created BEFORE it -> the
    conv consumer runs first (FAN_DONE), the gradient is returned as usual and the fan-out adds it.  Same result both ways.  (c) NO conv
    consumer registered itself for the fan-out (FAN_GEOM has no entry: C1's 3x3 conv reading a zero-padded copy that lost the fan tag), or
    the registered one reads another shape than the gradient's -> the gradient is returned, nothing is stashed, the fan-out adds it."""
    import fovealseg  # noqa: F401
    from fovealseg import ops

    log = []

    class ConvStandIn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, k):
            ctx.fan = getattr(x, "_fs_fan", None)
            ctx.k = k
            ops.FAN_GEOM[ctx.fan[0]] = ops.ConvProblem.of(x.shape, (1, 1, 1, 1), 1, 0)      # as ConvBnAct.forward registers the conv consumer
            return x * k

        @staticmethod
        def backward(ctx, g):
            pend = ops.PENDING_RES.pop(ctx.fan[0], None)
            ops.FAN_DONE.add(ctx.fan[0])
            log.append("conv+addend" if pend is not None else "conv")
            dx = g * ctx.k
            return (dx + pend[0] if pend is not None else dx), None

    def run(stash_after_conv):
        ops.reset_step_state()
        log.clear()
        x = torch.arange(8, dtype=torch.float32).view(2, 2, 2, 1).requires_grad_(True)
        h = x * 1.0                                    # a non-leaf, like the encoder's output
        fa, fb = ops.fan_out(h, 2)
        fan = fa._fs_fan
        if not stash_after_conv:
            fb = ops.StashGrad.apply(fb, fan[0])
        y1 = ConvStandIn.apply(fa, 3.0)
        if stash_after_conv:
            fb = ops.StashGrad.apply(fb, fan[0])
        y2 = (fb * fb).sum()
        (y1.sum() + y2).backward()
        assert not ops.PENDING_RES
        return x.grad.clone()

    want = 3.0 + 2.0 * torch.arange(8, dtype=torch.float32).view(2, 2, 2, 1)
    ga = run(True)
    assert log == ["conv+addend"], log
    gb = run(False)
    assert log == ["conv"], log
    assert torch.equal(ga, want) and torch.equal(gb, want)
    ops.reset_step_state()

    # (c) the other alias is read by something that never looks at PENDING_RES
    def run_without_conv_consumer(geom):
        ops.reset_step_state()
        x = torch.arange(8, dtype=torch.float32).view(2, 2, 2, 1).requires_grad_(True)
        h = x * 1.0
        fa, fb = ops.fan_out(h, 2)
        fan = fa._fs_fan
        if geom is not None:
            ops.FAN_GEOM[fan[0]] = geom
        y1 = fa * 3.0                                  # a plain consumer: pops nothing
        fb = ops.StashGrad.apply(fb, fan[0])
        y2 = (fb * fb).sum()
        (y1.sum() + y2).backward()
        assert not ops.PENDING_RES, "a gradient was stashed for a conv consumer that does not exist"
        ops.reset_step_state()                         # ... so the next forward has nothing to complain about
        return x.grad.clone()

    assert torch.equal(run_without_conv_consumer(None), want)
    padded = ops.ConvProblem.of((2, 2, 2, 16), (1, 16, 1, 1), 1, 0)
    assert torch.equal(run_without_conv_consumer(padded), want)      # a consumer of a padded copy: other shape


# ---- where the stateless ops live: frames / masks / gaze / overlay / unwarp beside ops (DESIGN.md "Where things live") ----------------
_OP_MODULES = ("frames", "masks", "gaze", "overlay", "unwarp")


@pytest.mark.parametrize("name", _OP_MODULES)
def test_op_module_names_resolve_through_ops(name):
    mod = getattr(fovealseg, name)
    assert mod.__all__ and len(set(mod.__all__)) == len(mod.__all__)
    for n in mod.__all__:
        assert not n.startswith("_")
        assert getattr(ops, n) is getattr(mod, n), n
    # every public thing the module defines is in its __all__: nothing is reachable there and missing from ops
    own = [n for n, v in vars(mod).items() if not n.startswith("_") and getattr(v, "__module__", mod.__name__) == mod.__name__
           and not isinstance(v, type(os))]
    assert sorted(n for n in own if n not in mod.__all__) == []


@pytest.mark.parametrize("name", _OP_MODULES)
def test_op_modules_do_not_import_ops(name):
    mod = getattr(fovealseg, name)
    assert "ops" not in vars(mod)
    assert not any(v is ops for v in vars(mod).values())


def test_frame_in_place():
    B, H, W = 2, 4, 6
    f32 = torch.rand(B, 3, H, W)
    planar = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8)
    hwc = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8).permute(0, 3, 1, 2)
    sliced = torch.randint(0, 256, (B, 3, H, 2 * W), dtype=torch.uint8)[..., ::2]
    nv12 = ops.Nv12Frame(torch.randint(0, 256, (B, H, W), dtype=torch.uint8), torch.randint(0, 256, (B, H // 2, W // 2, 2), dtype=torch.uint8),
                         matrix="bt601")
    assert ops.byte_frame_layout(hwc)[0] == "hwc" and ops.byte_frame_layout(sliced) is None and tuple(sliced.shape) == (B, 3, H, W)
    for img, stays in ((f32, False), (planar, False), (hwc, True), (nv12, True)):
        x, in_place = fovealseg.frames.frame_in_place(img)
        assert x is img and in_place is stays
    x, in_place = fovealseg.frames.frame_in_place(sliced)
    assert x is not sliced and x.is_contiguous() and torch.equal(x, sliced) and in_place is False
