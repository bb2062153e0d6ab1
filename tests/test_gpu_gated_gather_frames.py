"""
Stream ordering of the gathered frames: amt_gather_frames behind the gated side stream (tests/_gated_stream.py,
tests/_gated_gather_frames_cases.py), and GatherSequence.process issued on a current stream that is not the default one, with
device-resident images that only become true behind a gate on that stream.
"""
import numpy as np
import pytest

import _gated_gather_frames_cases as GK
import _gated_stream as GS
import _gather_frames_cases as FC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('n', [1, 3])
def test_gather_frames_behind_the_gate(n):
    case = GK.case(n)
    want, _, _ = GS.baseline(case)
    # the baseline is what the per-job calls give, so the gated run is compared with the right bytes
    res = FC.run([dict(FC.by_name(name), masked_columns=(20, 30) if k == GK.MASKED else None) for k, name in enumerate(GK.JOBS)],
                 np.uint16, 3, 'linear', n=n, min_count=max(1, (n * n + 1) // 2))
    for k, r in enumerate(res['jobs']):
        for key in ('img', 'mask', 'elev') + (('count',) if n > 1 else ()):
            assert np.array_equal(want['%s_%d' % (key, k)], r[key]), (n, k, key)
    GS.run_gated(case)


def test_process_on_a_side_stream_with_images_that_arrive_behind_a_gate():
    import torch
    from auromat_amd.pipeline import GatherSequence
    from auromat_amd.synthetic import frame_image, sequence_frame
    w, h, count = 265, 177, 5
    metas = [sequence_frame(k, w, h) for k in range(count)]
    true = [frame_image(w, h, seed=m[3]) for m in metas]
    decoy = [frame_image(w, h, seed=500 + k) for k in range(count)]
    seq = GatherSequence(w, h, pxPerDeg=10, batch=2)

    def frames(images):
        return [(m[0], m[1], m[2], img) for m, img in zip(metas, images)]

    settled = [GS.dev(a) for a in true]
    torch.cuda.synchronize()
    base = seq.process(frames(settled), keep_on_device=True)
    torch.cuda.synchronize()
    assert seq.plans == ['gather'] * count
    want = [{k: GS.bits(r[k]) for k in ('img', 'mask', 'elevation')} for r in base]
    assert all((b['mask'] == 0).any() for b in want)
    # behind a gate on a side stream: the images hold the decoys until copies on that stream replace them
    images = [GS.dev(a) for a in decoy]
    staging = [GS.dev(a) for a in true]
    with GS.Gate(GS.GATE_MS) as gate:
        for img, src in zip(images, staging):
            img.copy_(src)
        res = seq.process(frames(images), keep_on_device=True)
        snaps = [{k: r[k].clone() for k in ('img', 'mask', 'elevation')} for r in res]
    gate.side.synchronize()
    for k, (s, b) in enumerate(zip(snaps, want)):
        for key in b:
            assert np.array_equal(GS.bits(s[key]), b[key]), (k, key, 'the consumer on the side stream saw other bytes')
    torch.cuda.synchronize()
    # (and the decoys give other samples: the comparison above could tell)
    other = seq.process(frames([GS.dev(a) for a in decoy]), keep_on_device=False)
    assert not np.array_equal(other[0]['img'].view(np.uint8).reshape(-1), want[0]['img'])
