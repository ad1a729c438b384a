"""The cases of tests/pass_branch_cases.py as inputs (no GPU): the oracle alone, with its branch log on, must take on each case the
outcomes the case is there for, on at least MIN_PIXELS pixels (a searched draw: on the pixel it was searched for); over all cases
every outcome of the log must be taken somewhere, apart from those argued unreachable in pass_branch_cases; no case may leave a
non-finite value in a compared buffer. tests/test_gpu_pass_branches.py then compares the HIP passes with the oracle on these cases."""
import ctypes as C

import numpy as np
import pytest

import pass_branch_cases as pbc

CASES = pbc.cases()
WORDS = (("ris", 0, "RIS_BITS", "RIS_BIT"), ("final", 1, "FINAL_BITS", "FINAL_BIT"))


def test_branch_log_is_off_by_default_and_changes_nothing(oracle, blue_noise):
    case = next(c for c in CASES if c.name == "pan")
    desc, W, H = case.scene(), case.W, case.H
    runs, UNSET = [], 0xA5A5A5A5
    for logged in (False, True):
        osc = oracle.OracleScene().load(desc)
        of = oracle.HostFrame(W, H, blue_noise)
        log = np.full((H, W, 2), UNSET, dtype=np.uint32)
        prev, frames = None, []
        for fr in case.frames[:3]:
            m = oracle.camera_matrices(fr.camera[0], fr.camera[1], desc.fov_y, W, H, prev)
            prev = list(m.view_proj)
            if logged and fr.frame_count == 1:
                osc.set_branch_log(log)
            osc.trace_ris(of, m, fr.frame_count, fr.cfg)
            osc.trace_final(of, m, fr.frame_count, fr.cfg)
            frames.append(pbc.snapshot(of, fr.frame_count))
        c = osc.counters()
        runs.append((frames, log, (c.closest_queries, c.any_queries, c.boxes_tested, c.tris_tested)))
        osc.close()
    (a, untouched, ca), (b, log, cb) = runs
    assert (untouched == UNSET).all() and ca == cb
    for fa, fb in zip(a, b):
        for name in pbc.BUFFERS:
            assert fa[name].tobytes() == fb[name].tobytes(), name
    assert (log != UNSET).all() and (log[..., 0] != 0).any() and (log[..., 1] != 0).any()


def test_bit_names_fit_their_words(oracle):
    assert len(set(oracle.RIS_BITS)) == len(oracle.RIS_BITS) <= 32 and len(set(oracle.FINAL_BITS)) == len(oracle.FINAL_BITS) <= 32
    for word, _, names, _ in WORDS:
        assert pbc.UNREACHABLE[word] <= set(getattr(oracle, names))
        for case in CASES:
            assert set(case.want[word]) <= set(getattr(oracle, names)) - pbc.UNREACHABLE[word], case


@pytest.mark.parametrize("name", sorted(pbc.DRAWS))
def test_searched_frame_counts_draw_exactly_one(oracle, name):
    """DRAWS[name] = (x, y, k, frame_count): the k-th draw of the pixel's stream is a 32-bit result >= 0xFFFFFF80, which rnd() converts
    to 1.0f, and no earlier draw is; the search finds the committed constant again when started just below it."""
    x, y, k, frame_count = pbc.DRAWS[name]
    seed = oracle.lib().orc_init_rng(C.c_uint32(x), C.c_uint32(y), C.c_uint32(frame_count), C.c_uint32(pbc.DRAW_W))
    words, vals = (C.c_uint32 * (k + 1))(), (C.c_float * (k + 1))()
    oracle.lib().orc_rnd_stream(C.c_uint32(seed), C.c_uint32(k + 1), words, vals)
    assert words[k] >= 0xFFFFFF80 and vals[k] == 1.0 and all(v < 1.0 for v in list(vals)[:k])
    assert pbc.find_draw_frames(x, y, pbc.DRAW_W, {k}, start=max(frame_count - 1000, 0), chunk=2048) == {k: frame_count}


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_reaches_the_outcomes_it_is_there_for(oracle, blue_noise, case):
    """head_on: only the centre pixel of an odd extent can look along the normal bit for bit (pass_branch_cases.head_on_quad), so that
    case names its pixel as the searched draws do, and must show the outcome there in every one of its frames."""
    assert case.scene().n_triangles() <= 400
    recs = pbc.oracle_frames(oracle, case, blue_noise)
    for word, k, names, table in WORDS:
        names, table = getattr(oracle, names), getattr(oracle, table)
        counts = {n: 0 for n in names}
        for rec in recs:
            for n, v in pbc.count_bits(rec["log"][..., k], names, table).items():
                counts[n] += v
        print(case.name, word, {n: v for n, v in counts.items() if v})
        for n in pbc.UNREACHABLE[word]:
            assert counts[n] == 0, "%s: '%s' is argued unreachable, yet %d pixels took it" % (case.name, n, counts[n])
        for n in case.want[word]:
            if case.pixel is None:
                assert counts[n] >= pbc.MIN_PIXELS, "%s: %s outcome '%s' on %d pixels" % (case.name, word, n, counts[n])
            else:
                x, y, f = case.pixel
                for rec in (recs if f is None else [recs[f]]):
                    assert rec["log"][y, x, k] & table[n], "%s: %s outcome '%s' not taken at pixel (%d, %d)" % (case.name, word, n, x, y)


def test_update_draw_leaves_weight_without_a_sample(oracle, blue_noise):
    """The state p_hat_held's "no sample taken = the zero sample" rests on (ris_kernel): the single candidate of the searched pixel has a
    weight and is not taken, so the reservoir keeps position and normal 0 with w_sum > 0; its W is w_sum / 1e-4 (target value 0 under
    the floor of the division), and it survives the visibility test because the origin is in front of the back wall and in sight."""
    case = next(c for c in CASES if c.name == "draw_one_ris_update")
    x, y, _, _ = pbc.DRAWS[case.name]
    r = pbc.oracle_frames(oracle, case, blue_noise)[0]["after_ris"]["reservoirs"][y * case.W + x]
    assert r["w_sum"] > 0 and r["M"] == 1 and not r["light_pos"].any() and not r["light_normal"].any()
    assert r["W"] == np.float32(r["w_sum"]) / np.float32(1e-4)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_leaves_only_finite_values(oracle, blue_noise, case):
    """x86 and the GPU give NaNs different bit patterns: a compared buffer may hold none. Infinity is a pattern some cases inject;
    what the passes write must be finite."""
    for rec in pbc.oracle_frames(oracle, case, blue_noise):
        for stage in ("after_ris", "after_final"):
            snap = rec[stage]
            assert np.isfinite(snap["raw_color"]).all(), stage
            for buf in ("reservoirs", "reservoirs_gi"):
                for field in snap[buf].dtype.names:
                    a = snap[buf][field]
                    if a.dtype.kind == "f":
                        assert not np.isnan(a).any(), (stage, buf, field)
                        if stage == "after_ris":
                            assert np.isfinite(a).all(), (stage, buf, field)
            assert not ((snap["depth"] & 0x7FFF) > 0x7C00).any() and not ((snap["motion"] & 0x7FFF) > 0x7C00).any()
            assert not (((snap["motion"] >> 16) & 0x7FFF) > 0x7C00).any()


def test_every_outcome_is_taken_by_some_case(oracle, blue_noise):
    for word, k, names, table in WORDS:
        names, table = getattr(oracle, names), getattr(oracle, table)
        seen = np.uint32(0)
        for case in CASES:
            for rec in pbc.oracle_frames(oracle, case, blue_noise):
                seen |= np.bitwise_or.reduce(rec["log"][..., k].reshape(-1))
        missing = {n for n in names if not int(seen) & table[n]}
        assert missing == pbc.UNREACHABLE[word], (word, sorted(missing))
        wanted = {n for case in CASES for n in case.want[word]}
        assert wanted == set(names) - pbc.UNREACHABLE[word], (word, sorted(set(names) - pbc.UNREACHABLE[word] - wanted))
