"""DynamicPipeline(solo_head=f, solo_input=...) over the 12-frame rendered 640 x 360 scene of tests/test_solo_head.py: the callable is handed each frame's
[3, model_h, model_w] device tensor, checked here against the restatement within the bar, and the run equals the same run without solo_input bit for bit — rows,
object rows, trajectory, object states and statistics.  The keyword is refused without solo_head."""
import numpy as np
import pytest

from tests import solo_input_ref as sr

MODEL = (320, 192)          # 640 x 360 -> rect (0, 6, 320, 180): pads above and below


def test_keyword_is_refused_without_solo_head():
    from dynamic_vins_amd.pipeline import DynamicPipeline
    with pytest.raises(ValueError, match="solo_input needs solo_head"):
        DynamicPipeline(None, solo_input=MODEL)
    with pytest.raises(ValueError, match="solo_input must be"):
        DynamicPipeline(None, solo_head=lambda k, x: None, solo_input=(320,))


@pytest.mark.gpu
def test_pipeline_with_input_equals_the_run_without():
    from dynamic_vins_amd.pipeline import DynamicPipeline
    from tests.test_inst_stack import KW, runner_sequence
    from tests.test_solo_head import scene_head
    seq, steps = runner_sequence(), 12
    assert (seq.w, seq.h) == (640, 360) and sr.rect(*MODEL, seq.w, seq.h) == (0, 6, 320, 180)

    def run(with_input):
        log, seen = [], []
        head = scene_head(seq, log)

        def head_with_input(k, inp):
            assert tuple(inp.shape) == (3, MODEL[1], MODEL[0]) and inp.is_cuda and inp.is_contiguous()
            gray = seq.frames[k][0].cpu().numpy()
            r = sr.solo_input(np.repeat(gray[:, :, None], 3, axis=2), *MODEL)
            got = inp.cpu().numpy()
            d = float(np.abs(got.astype(np.float64) - r["out"]).max())
            assert d <= sr.BAR and not got[:, ~r["inside"]].view(np.uint32).any(), (k, d)
            seen.append((k, inp.data_ptr(), d))
            return head(k)
        p = DynamicPipeline(seq, solo_head=head_with_input, solo_input=MODEL, **KW) if with_input else DynamicPipeline(seq, solo_head=head, **KW)
        rows = []
        for _ in range(steps):
            p.step()
            rows.append((p.rows.tobytes(), np.asarray(p.ifeats).tobytes()))
        I, S = p.est.instances()
        res = (rows, np.asarray(p.poses).tobytes(), I.tobytes(), np.asarray(S).tobytes(), dict(p.stat))
        p.ctx.close()
        return res, seen

    a, seen = run(True)
    assert [k for k, _, _ in seen] == list(range(len(seen))) and len(seen) > steps
    assert all(seen[i][1] != seen[i + 1][1] for i in range(len(seen) - 1)) and len({s[1] for s in seen}) == 2, "the inputs do not alternate between two buffers"
    print("device - restatement over %d frames: %.3g" % (len(seen), max(s[2] for s in seen)))
    b, _ = run(False)
    assert a[4]["object_features"] > 50, a[4]
    assert a == b
