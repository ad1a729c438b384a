"""The history-reach check's range against the reads the RIS pass really makes (no GPU): the oracle logs, per pixel of a
moving-camera frame, the history pixel it computes for the DI and the GI reservoir; each must lie in the range the check's
restatement derives from the motion vector stored for that pixel. Extents 1920 x 8 and 8 x 1080 put a half-precision motion vector
up to half a pixel off along the long axis."""
import numpy as np
import pytest

import history_read_util as hr
import strip_reference as ref


def test_read_log_is_off_by_default_and_changes_nothing(oracle, blue_noise):
    from oracle.binding import NO_READ
    desc = hr.SCENES["cornell_glass_mirror"]()
    W, H = 48, 32
    frames, UNSET = [], -12345
    for logged in (False, True):
        osc = oracle.OracleScene().load(desc)
        of = oracle.HostFrame(W, H, blue_noise)
        log = np.full((H, W, 4), UNSET, dtype=np.int32)
        prev = None
        for f in range(2):
            m = oracle.camera_matrices((0.1 * f, 1.0, 3.4), desc.camera_target, desc.fov_y, W, H, prev)
            prev = list(m.view_proj)
            if logged and f == 1:
                osc.set_read_log(log)
            osc.trace_ris(of, m, f)
            osc.trace_final(of, m, f)
        frames.append((of, log))
        osc.close()
    (a, untouched), (b, log) = frames
    assert (untouched == UNSET).all()
    for name in ("motion", "depth", "normal", "diffuse", "raw_color"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert a.reservoirs[1].tobytes() == b.reservoirs[1].tobytes() and a.reservoirs_gi[1].tobytes() == b.reservoirs_gi[1].tobytes()
    assert (log != UNSET).all() and (log[..., 0] != NO_READ).any() and (log[..., 2] != NO_READ).any()


@pytest.mark.parametrize("scene_name", sorted(hr.SCENES))
def test_every_logged_read_lies_in_the_range_of_its_stored_motion_vector(oracle, blue_noise, scene_name):
    smallest = None
    for W, H, axes in ((1920, 8, (True,)), (8, 1080, (False,)), (120, 48, (True, False))):
        for cols in axes:
            for label, cam in hr.camera_moves(oracle, scene_name, W, H, cols, blue_noise):
                motion, log = hr.ris_pair(oracle, scene_name, W, H, cam, blue_noise)
                slack, n = hr.read_slack(motion, log, cols)
                px = hr.axis_motion_pixels(motion, cols)
                print("%s %dx%d %s %s: %d reads, smallest slack %s px, stored motion median %.2f / largest %.2f px" % (
                    scene_name, W, H, "cols" if cols else "rows", label, n, slack, np.median(px), px.max()))
                assert n > 0, "no history read inside the image"
                smallest = slack if smallest is None else min(smallest, slack)
    assert smallest <= 1, "no read near an end of its range: the comparison says little (smallest slack %d px)" % smallest


def test_slack_check_sees_a_range_without_its_margin(oracle, blue_noise, monkeypatch):
    """The comparison itself: with the one-pixel margin taken off both ends of the range, reads fall outside it."""
    cam = hr.camera_moves(oracle, "cornell_glass_mirror", 120, 48, True, blue_noise)[2][1]
    motion, log = hr.ris_pair(oracle, "cornell_glass_mirror", 120, 48, cam, blue_noise)
    real = ref.reach_f32

    def short(m, pos, n, cols, clip=True):
        kind, lo, hi = real(m, pos, n, cols, clip)
        return kind, lo + 1, hi - 1
    monkeypatch.setattr(ref, "reach_f32", short)
    with pytest.raises(AssertionError, match="outside"):
        hr.read_slack(motion, log, True)
