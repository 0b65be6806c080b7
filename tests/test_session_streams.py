"""GazeSession held to a numpy model of itself over long seeded streams.

tests/session_ref.py restates the session (RefSession), gives it a stub head whose record is a pure integer function of one viewer's
frame and gaze (stub_record; StubModule on the device), and draws seeded streams: cameras that translate, jump and cut over textured
canvases, gazes that follow, drift, leave the mask and jump, forces, resets, and a frame layout that changes every step.  Every
comparison is bit equality.  The CPU tests hold the model's sliced moves to motion_ref's loops, the stub's twin to hand-derived records,
and assert that every configuration's stream reaches what it is there for; the GPU tests hold the device session to the model after
every step -- the returned record, gate, motion, the counts dict and the private state -- and to invariants that do not come from the
step order."""
import numpy as np
import pytest
import torch

import gate_ref as R
import motion_ref as M
import rle_ref as RLE
import session_ref as S
from test_gaze_session import served                     # noqa: F401  (a fixture)

from fovealseg.session import GazeSession


# ------------------------------------------------------------------------------------------------------------------ CPU: the moves ---
@pytest.mark.parametrize("H,W", [(9, 37), (12, 64)])
def test_sliced_moves_equal_the_loops(H, W):
    rng = np.random.default_rng(H * 100 + W)
    mask = rng.random((H, W)) < 0.5
    key = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    img = rng.random((3, H, W), dtype=np.float32) * 1.5 - 0.25
    img[0, 1, 2] = np.float32("nan")
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            assert np.array_equal(S.move_mask(mask, dy, dx), M.move_mask(mask, dy, dx)), (dy, dx)
            assert np.array_equal(S.move_key(key, img, dy, dx), M.move_key(key, img, dy, dx)), (dy, dx)
    for dy, dx in ((H, 0), (0, -W), (H + 2, W + 2)):      # everything leaves
        assert not S.move_mask(mask, dy, dx).any() and np.array_equal(S.move_key(key, img, dy, dx), R.q(img).astype(np.uint8))


def test_state_shift_of_the_model_equals_motion_ref():
    rng = np.random.default_rng(3)
    B, H, W, cap = 3, 9, 37, 7
    masks = rng.random((B, H, W)) < 0.4
    img = rng.random((B, 3, H, W), dtype=np.float32)
    key = rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8)
    st = dict(key=key, bits=np.stack([RLE.bits(m) for m in masks]), gstate=rng.integers(0, 16 * 8, (B, 6)),
              stats=np.array([RLE.stats(m) for m in masks], dtype=np.int64), counts=np.stack([RLE.counts_row(m, cap) for m in masks]),
              prof_key=M.key_profiles(key), mstate=rng.integers(-9, 9, (B, 4)))
    shift = np.array([[2, -3, 5, 9], [0, 0, 1, 1], [-1, 0, 0, 4]], dtype=np.int64)
    want = M.state_shift(img, shift, *st.values())
    got = S.state_shift(img, shift, *st.values())
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and sorted(got[-1]) == [0, 2]


# ------------------------------------------------------------------------------------------------------------------ CPU: the stub ----
def test_stub_record_of_a_dark_frame_is_the_empty_record():
    H, W, cap = 12, 20, 9
    cat, stats, counts, bits, conf = S.stub_record(np.zeros((3, H, W), dtype=np.float32), np.array([0.5, 0.5], dtype=np.float32), H, W, cap, True)
    # the gaze: rint(0.5 * 11 * 16) = 88 -> pixel (88 + 8) >> 4 = 6; rint(0.5 * 19 * 16) = 152 -> pixel 10
    assert int(cat) == (31 * 6 + 17 * 10) % 50 == 6
    assert stats.tolist() == [0, 0, 0, 0, 0, 1] and counts.tolist() == [H * W] + [0] * 8 and not bits.any() and bits.shape == (H, 1)
    assert conf.tolist() == [0.0, 0.0, 6.0]


def test_stub_record_of_a_bright_frame_is_the_clipped_square():
    H, W, cap = 12, 40, 9                                # r = 3; the gaze in the bottom right corner: rows 8 .. 11, columns 36 .. 39
    cat, stats, counts, bits = S.stub_record(np.ones((3, H, W), dtype=np.float32), np.array([1.0, 1.0], dtype=np.float32), H, W, cap, False)
    assert int(cat) == (31 * 11 + 17 * 39) % 50 == 4
    assert stats.tolist() == [16, 36, 8, 4, 4, 8]
    assert counts.tolist() == [36 * 12 + 8, 4, 8, 4, 8, 4, 8, 4, 0]                      # four columns of four set pixels, the last to the end
    assert bits[:8].tolist() == [[0, 0]] * 8 and bits[8:].tolist() == [[0, 0xF0]] * 4    # bits 4 .. 7 of the second word
    # the top left corner, with the score: L = 765 under the gaze, area 16
    cat, stats, counts, bits, conf = S.stub_record(np.ones((3, H, W), dtype=np.float32), np.array([0.0, 0.0], dtype=np.float32), H, W, cap, True)
    assert stats.tolist() == [16, 0, 0, 4, 4, 9] and counts.tolist() == [0, 4, 8, 4, 8, 4, 8, 4, 12 * 36 + 8]
    assert conf.tolist() == [765.0, 16.0, 0.0]


def test_stub_record_of_one_bright_pixel_under_the_gaze():
    H, W, cap = 12, 20, 9
    img = np.zeros((3, H, W), dtype=np.float32)
    img[:, 6, 10] = 0.5                                  # q = 128 a channel: L = 384 >= 383
    img[:, 6, 11] = (0.5, 0.5, 0.496)                    # 128 + 128 + rint(126.48) = 382: below the threshold
    cat, stats, counts, bits, conf = S.stub_record(img, np.array([0.5, 0.5], dtype=np.float32), H, W, cap, True)
    assert stats.tolist() == [1, 10, 6, 1, 1, 3] and counts.tolist() == [10 * 12 + 6, 1, 12 * 20 - 127] + [0] * 6
    assert bits[6].tolist() == [1 << 10] and int(np.count_nonzero(bits)) == 1 and conf.tolist() == [384.0, 1.0, 6.0]
    img[:, 2, 10] = 1.0                                  # four rows above the gaze: outside r = 3
    assert S.stub_record(img, np.array([0.5, 0.5], dtype=np.float32), H, W, cap, False)[1].tolist() == [1, 10, 6, 1, 1, 3]


def test_model_frame_layouts():
    rgba = np.arange(2 * 3 * 5 * 4, dtype=np.uint8).reshape(2, 3, 5, 4)                 # every alpha value 3, 7, .. once: 3 is wild
    plain = S.model_frame(rgba, "hwc")
    assert plain.shape == (2, 3, 3, 5) and np.array_equal(R.q(plain), rgba[..., :3].transpose(0, 3, 1, 2))
    wild = S.model_frame(rgba, "wild")
    assert np.isinf(wild[0, 0, 0, 0]) and np.array_equal(wild[:, 1:], plain[:, 1:]) and int((wild != plain).sum()) == 1


# ------------------------------------------------------------------------------------------------------------------ CPU: coverage ----
# the codes a configuration can reach.  RUN_AGE needs max_age, HOLD_SACCADE a saccade threshold.  D has scene_frac = 0: a changed
# tile in the region of interest is a changed tile, and RUN_SCENE comes first in the gate's order -- RUN_ROI cannot occur.
CODES = {"A": set(range(8)), "B": set(range(8)) - {R.RUN_AGE}, "C": set(range(8)) - {R.RUN_AGE, R.HOLD_SACCADE},
         "D": set(range(8)) - {R.RUN_AGE, R.RUN_ROI}}


def _moving(name):
    return S.CONFIGS[name]["kw"].get("motion_px")


def _gate(st, moving):
    return st["out"][-2] if moving else st["out"][-1]


def coverage(name):
    """What the stream of a configuration reaches, counted from the model's trace alone."""
    c, steps = S.CONFIGS[name], S.trace(name)
    B, Rm = c["B"], _moving(name)
    n = dict(codes={k: 0 for k in range(8)}, all_run=0, all_run_then_move=0, idle=0, subset=0, moves=0, both=0, full=0, rejected=0, shrink=0,
             clamp=0, move_and_run=0, move_beside_reset=0, cut_code_moved=0, subset_of_a_view=0, remade_after_moves=0, hold_after_move=0,
             pairs=set())
    moved_at, last_moved = [], set()
    for t, st in enumerate(steps):
        gate = _gate(st, Rm)
        for code in gate[:, 0].tolist():
            n["codes"][code] += 1
        ran = st["ran"]
        n["all_run"] += len(ran) == B
        n["idle"] += not ran
        n["subset"] += 0 < len(ran) < B
        n["subset_of_a_view"] += 0 < len(ran) < B and S.HEAD_SEES[st["layout"]] == "hwc"    # byte_frame_select's steps
        moved = set()
        if Rm:
            motion = st["out"][-1]
            for b in range(B):
                dy, dx = int(motion[b, 0]), int(motion[b, 1])
                if (dy, dx) == (0, 0):
                    n["rejected"] += int(motion[b, 2]) < int(motion[b, 3])             # a better shift was found and not taken
                    continue
                moved.add(b)
                before, after, n_runs, clamped = st["diag"][b]
                n["moves"] += 1
                n["both"] += dy != 0 and dx != 0
                n["full"] += max(abs(dy), abs(dx)) == Rm
                n["shrink"] += 0 < after < before
                n["clamp"] += clamped
                n["move_and_run"] += b in ran
                n["move_beside_reset"] += st["reset"] is not None and b not in st["reset"] and any(v in st["reset"] for v in (b - 1, b + 1))
                n["cut_code_moved"] += n_runs > (c["kw"].get("max_runs") or 10 ** 9)
            for b in range(B):
                carried = int(steps[t - 1]["state"]["mstate"][b, 2]) if t else 0        # the moves the record had behind it
                n["remade_after_moves"] += int(gate[b, 0]) in (R.RUN_INIT, R.RUN_FORCED) and carried >= 2
                n["hold_after_move"] += int(gate[b, 0]) == R.HOLD_SACCADE and (b in moved or b in last_moved)
        last_moved = moved
        moved_at.append(bool(moved))
        if t:
            n["pairs"].add((steps[t - 1]["layout"], st["layout"]))
    n["all_run_then_move"] = sum(len(st["ran"]) == B and any(moved_at[t + 1:t + 4]) for t, st in enumerate(steps))
    return n


@pytest.mark.parametrize("name", sorted(S.CONFIGS))
def test_streams_reach_what_they_are_there_for(name):
    """Conditions on the inputs, met by the model alone."""
    c, n = S.CONFIGS[name], coverage(name)
    B, Rm = c["B"], _moving(name)
    print(name, {k: v for k, v in n.items() if k != "pairs"}, len(n["pairs"]))
    assert all(n["codes"][k] >= 3 for k in CODES[name]), n["codes"]
    assert all(n["codes"][k] == 0 for k in set(range(8)) - CODES[name]), n["codes"]
    assert sum(n["codes"].values()) == B * c["steps"]
    assert n["all_run"] >= 1 and n["idle"] >= 10
    if B > 1:
        assert n["subset"] >= 10 and n["subset_of_a_view"] >= 3
    layouts = S.LAYOUTS + (("expand",) if B == 1 else ())
    assert {(a, b) for a in layouts for b in layouts if a != b} <= n["pairs"]
    if not Rm:
        return
    assert n["all_run_then_move"] >= 1
    assert n["moves"] >= 15 and n["both"] >= 3 and n["full"] >= 2 and n["shrink"] >= 1 and n["clamp"] >= 1 and n["move_and_run"] >= 1
    assert n["remade_after_moves"] >= 1                  # a reset or a force on a record carried two moves or more
    if R.HOLD_SACCADE in CODES[name]:
        assert n["hold_after_move"] >= 1                 # a saccade in flight in the step of a move or the step after one
    if c["kw"].get("motion_gain", 6) < 8:                # at gain 8 the rule is cost <= cost(0), which the least cost always meets
        assert n["rejected"] >= 1
    if B > 1:                                            # one viewer has no neighbour
        assert n["move_beside_reset"] >= 1
    if name == "C":
        assert n["cut_code_moved"] >= 1


def test_the_model_counts_and_resets_like_the_session():
    """The host side of the model on a scene small enough to follow by hand: two viewers, a dark frame, nothing moves."""
    H, W = 16, 24
    m = S.RefSession(S.stub_predict(H, W, 8 * W + 1, False), 2, (H, W), tile=8, max_age=2)
    img, f = np.zeros((2, 3, H, W), dtype=np.float32), np.full((2, 2), 0.5, dtype=np.float32)
    codes = []
    for t in range(5):
        if t == 3:
            m.reset([1])
        codes.append(m.step(img, f, [1, 0] if t == 1 else None)[-1][:, 0].tolist())
    # viewer 0: init, forced, reuse, reuse, age (age + 1 = 3 > 2); viewer 1: init, reuse, reuse, init after the reset, reuse
    assert codes == [[1, 1], [7, 0], [0, 0], [0, 1], [6, 0]]
    assert m.counts == {0: 5, 1: 3, 2: 0, 3: 0, 4: 0, 5: 0, 6: 1, 7: 1}
    assert m.gstate[:, 5].tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------------------------ GPU --------------
def _np(t):
    return t.detach().cpu().numpy()


def _bits_equal(a, b):
    """Two arrays bit for bit: fp32 is compared as its words, so that NaN equals NaN and -0 differs from 0."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32 or b.dtype == np.float32:
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(S.CONFIGS))
def test_stub_module_equals_its_twin(name):
    c = S.CONFIGS[name]
    B, H, W, kw = c["B"], c["H"], c["W"], c["kw"]
    score, cap = bool(kw.get("score")), (8 * W + 1 if kw.get("max_runs") is None else kw["max_runs"])
    n = 3
    rgba = np.stack([np.concatenate([S._canvas_bytes(77 + j, H, W)[:, j:j + H, 2 * j:2 * j + W].transpose(1, 2, 0),
                                     np.arange(H * W, dtype=np.uint8).reshape(H, W, 1)], axis=2) for j in range(n)])
    focus = np.array([[0.5, 0.5], [0.0, 1.0], [0.97, 0.31]], dtype=np.float32)
    for layout in ("wild", "u8", "rgba"):
        img = S.model_frame(rgba, layout)
        want = S.stub_predict(H, W, cap, score)(img, focus)
        assert 0 < int(want[1][0, 0]) < (2 * (min(H, W) // 4) + 1) ** 2, "the seeded frame must give a mask neither empty nor full"
        got = S.StubModule().predict_instances(S.device_frame(rgba, layout), torch.from_numpy(focus).cuda(), max_runs=kw.get("max_runs"),
                                               return_bits=True, return_score=score, component=kw.get("component"))
        assert len(got) == len(want) + (kw.get("component") is not None)
        for g, w in zip(got, want):
            assert _bits_equal(_np(g), w), (name, layout)


def _check_step(t, s, st, out, x, x_before, f, acc, moving, cap, score):
    """One step of a device session on the stub head against the model's trace and against the invariants."""
    B, H, W = s.batch, s.H, s.W
    where = f"step {t} ({st['layout']})"
    # --- the model ---
    assert len(out) == len(st["out"]), where
    names = ["cat", "stats", "counts", "bits"] + (["conf"] if score else []) + ["gate"] + (["motion"] if moving else [])
    for k, (g, w) in enumerate(zip(out, st["out"])):
        assert _bits_equal(_np(g), w), f"{where}: returned {names[k]}"
    assert s.counts == st["counts"], f"{where}: counts"
    state = dict(key=s._key, gstate=s._gstate, sad=s._sad)
    if moving:
        state.update(prof=s._prof, prof_key=s._prof_key, mstate=s._mstate)
    for k, v in state.items():
        assert _bits_equal(_np(v).astype(st["state"][k].dtype), st["state"][k]), f"{where}: _{k}"
    # --- the invariants ---
    gate = out[-2] if moving else out[-1]
    stats, counts, bits, key = _np(out[1]), _np(out[2]), _np(out[3]), _np(s._key)
    ran = [b for b in range(B) if int(gate[b, 0]) in R.RUNS]
    for b in range(B):
        mask = RLE.unbits(bits[b], W)
        assert stats[b].tolist() == RLE.stats(mask) and np.array_equal(counts[b], RLE.counts_row(mask, cap)), f"{where}: the code of viewer {b}'s bits"
    if moving:
        valid = _np(s._gstate)[:, 0] != 0
        assert np.array_equal(_np(s._prof_key).astype(np.int64)[valid], M.key_profiles(key)[valid]), f"{where}: the key's profiles"
        motion = _np(out[-1])
        for b in range(B):
            acc[b] = [0, 0] if b in ran else [acc[b][0] + int(motion[b, 0]), acc[b][1] + int(motion[b, 1])]
        assert motion[:, 4:].tolist() == acc, f"{where}: the totals"
    for b in ran:
        want = S.stub_record(st["img"][b], st["focus"][b], H, W, cap, score)
        for g, w in zip(out, want):
            assert _bits_equal(_np(g[b]), np.asarray(w)), f"{where}: viewer {b} ran"
        assert np.array_equal(key[b], R.q(st["img"][b])), f"{where}: the key of viewer {b}"
    assert _bits_equal(_np(x), x_before) and _bits_equal(_np(f), st["focus"]), f"{where}: the inputs were written"
    assert sum(s.counts.values()) == B * (t + 1)
    return ran


def run_stream(name, session_type=GazeSession, first_only=False):
    """The device session of a configuration over its stream, every step checked; returns the stub's call sizes."""
    c, steps = S.CONFIGS[name], S.trace(name)
    B, H, W, kw = c["B"], c["H"], c["W"], c["kw"]
    moving, score = kw.get("motion_px") is not None, bool(kw.get("score"))
    cap = 8 * W + 1 if kw.get("max_runs") is None else kw["max_runs"]
    stub = S.StubModule()
    s = session_type(stub, B, (H, W), **kw)
    acc = [[0, 0] for _ in range(B)]
    calls = []
    for t, st in enumerate(steps):
        if st["reset"] is not None:
            s.reset(None if len(st["reset"]) == B else st["reset"])
        x, f = S.device_frame(st["rgba"], st["layout"]), torch.from_numpy(st["focus"]).cuda()
        x_before = _np(x)
        force = st["force"] if st["force"] is None or t % 2 == 0 else torch.tensor(st["force"])
        out = s.step(x, f, force)
        ran = _check_step(t, s, st, out, x, x_before, f, acc, moving, cap, score)
        assert ran == st["ran"]
        calls += [len(ran)] if ran else []
        assert stub.calls == calls, f"step {t}: the head ran on {stub.calls[len(calls) - 1:]} viewers, {len(ran)} had a RUN code"
        if ran:                                          # the rows that run stay what the caller handed over: bytes stay bytes, a view a view
            assert stub.seen[-1] == S.HEAD_SEES[st["layout"]], f"step {t} ({st['layout']}): the head was handed {stub.seen[-1]} frames"
    return stub.calls


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(S.CONFIGS))
def test_session_equals_the_model_over_a_stream(name):
    calls = run_stream(name)
    assert len(calls) == sum(bool(st["ran"]) for st in S.trace(name))


REAL = dict(B=3, size=256, steps=16, seed=9, kw=dict(motion_px=8, score=True),
            # an eventful draw: sixteen steps have to hold moves, forces, cuts and a gaze that leaves, for three viewers
            probs=dict(run=0.25, jump=0.03, cut=0.06, flip=0.05, noise=0.05, jitter=0.08, on_set=0.03, on_clear=0.08, saccade=0.05, edge=0.0,
                       force=0.12, reset=0.10, reset_beside_run=0.15))


def _real_stream(model):
    return S.stream(REAL["seed"], REAL["B"], REAL["size"], REAL["size"], REAL["steps"], 8, tile=32, model=model, layouts=S.BYTE_LAYOUTS,
                    probs=REAL["probs"])


def test_the_real_network_stream_asks_for_subsets():
    """A condition on the inputs of test_session_equals_the_planar_path_with_the_real_head, as far as it can be had without the head:
    every byte layout occurs, and on two steps or more of an interleaved layout some viewers are forced -- they run whatever the record
    is -- and some are not.  That a strict subset did run there is asserted by the GPU test itself."""
    items = list(_real_stream(None))
    assert {it[4] for it in items} == set(S.BYTE_LAYOUTS)
    forced = [t for t, it in enumerate(items) if it[2] is not None and 0 < sum(it[2]) < REAL["B"] and it[4] != "u8"]
    assert len(forced) >= 2, forced


@pytest.mark.gpu
def test_session_equals_the_planar_path_with_the_real_head(served):
    """The real network in a stream of byte layouts: the session's subset path (index_select, byte_frame_select) against
    predict_instances on a planar fp32 copy of the rows that ran."""
    module, calls, TP = served
    B, size = REAL["B"], REAL["size"]

    def predict(img, focus):
        got = module.predict_instances(torch.from_numpy(np.ascontiguousarray(img)).cuda(), torch.from_numpy(np.ascontiguousarray(focus)).cuda(),
                                       return_bits=True, return_score=True)
        return [_np(g) for g in got]

    model = S.RefSession(predict, B, (size, size), **REAL["kw"])
    s = GazeSession(module, B, (size, size), **REAL["kw"])
    subsets = 0
    for t, (rgba, focus, force, reset, layout) in enumerate(_real_stream(model)):
        if reset is not None:
            model.reset(reset)
            s.reset(reset)
        want = model.step(S.model_frame(rgba, layout), focus, force)
        got = s.step(S.device_frame(rgba, layout), torch.from_numpy(focus).cuda(), force)
        assert len(got) == len(want) == 7
        for k, (g, w) in enumerate(zip(got, want)):
            assert _bits_equal(_np(g), np.asarray(w)), f"step {t} ({layout}): element {k}"
        assert s.counts == model.counts
        subsets += 0 < len(model.ran) < B and layout != "u8"
    print(f"counts {s.counts}, {subsets} steps ran a strict subset of an interleaved frame")
    assert subsets >= 1, "the stream must run a strict subset of the viewers on an interleaved frame"
