"""The order in which the native runner dispatches its kernels, for comparing two builds of the library (``AMT_LIB_PATH``).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/runner_kernel_order.py
    python3 tools/runner_kernel_order.py --list DIR OUT.txt

The first form runs five fixed small sequences (14 frames of 1060 x 708, batch 3, two calls each) through ``SequencePipeline``:
the mean with pxPerDeg, the mean with arcsecPerPx (box-first plan), the median, the area-weighted mean, and the mean from pinned
host images (more frames than slots); a torch ``cos_`` kernel marks the start of every call.  The second form writes the kernel
names of the trace in dispatch order, one per line, each with its stream numbered by first appearance — a host with one
dispatching thread gives the same listing run after run, so two builds are compared with ``diff``."""
import csv, glob, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def probe():
    import numpy as np
    import torch
    from auromat_amd.pipeline import SequencePipeline
    from auromat_amd.synthetic import frame_image, sequence_frame
    w, h, n = 1060, 708, 14
    imgs = [torch.from_numpy(frame_image(w, h, seed=100 + k).view(np.int16)) for k in range(n)]
    hdrs = [sequence_frame(k, w, h)[:3] for k in range(n)]
    dev = [hd + (im.cuda(),) for hd, im in zip(hdrs, imgs)]
    pin = [hd + (im.pin_memory(),) for hd, im in zip(hdrs, imgs)]
    mark = torch.zeros(64, device='cuda')
    for name, kw, feed in (('mean-ppd', dict(pxPerDeg=6), dev), ('mean-arcsec', dict(arcsecPerPx=600), dev),
                           ('median', dict(pxPerDeg=6, statistic='median'), dev), ('area', dict(pxPerDeg=6, statistic='area'), dev),
                           ('pinned', dict(pxPerDeg=6, own_image_buffers=True), pin)):
        seq = SequencePipeline(w, h, batch=3, **kw)
        for rep in range(2):
            mark.cos_()
            torch.cuda.synchronize()
            got = seq.process(feed, keep_on_device=True)
            torch.cuda.synchronize()
        print(name, 'frames', sum(1 for r in got if r is not None), 'plans', sorted(set(seq.plans)), flush=True)


def listing(trace_dir, out_path):
    path = glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True)[0]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Dispatch_Id']))
    streams = {}
    with open(out_path, 'w') as out:
        for r in rows:
            out.write('s%d %s\n' % (streams.setdefault(r.get('Stream_Id', r['Queue_Id']), len(streams)), r['Kernel_Name']))
    print(path, len(rows), 'kernels on', len(streams), 'streams')


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--list':
        listing(sys.argv[2], sys.argv[3])
    else:
        probe()
