"""
The mesh resampling kernels (k_mesh_claim, k_mesh_sample of auromat_amd/csrc/amt_mesh.hip) on constructed lattices and grids: the
cases of tests/_mesh_cases.py go to ``amt_mesh_frame`` as plain device arrays, and every byte of all four outputs (mesh, img,
mask, triangle) must equal tests/_mesh_oracle.py.  There is no tolerance anywhere: the oracle restates the kernels' arithmetic
operation for operation.  tests/test_mesh_cpu.py checks without a GPU that the oracle is right (scipy, rational arithmetic,
known answers) and that the cases aim where they claim to: the lane path, the wave path and the boundary between them, folds
and shared edges, the seam, the wrap, masks, grids coarser and far finer than the lattice.
"""
import ctypes as C

import numpy as np
import pytest

import _mesh_cases as K
import _mesh_oracle as O

pytestmark = pytest.mark.gpu

POISON = 0xA5
OUT_KEYS = ('mesh', 'img', 'mask', 'triangle')


def _device_array(a, offset=0):
    """A host array as a flat device tensor that starts `offset` elements into its allocation."""
    import torch
    from auromat_amd._native import Context
    a = np.ascontiguousarray(a).reshape(-1)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    whole = torch.empty(a.size + 2 * offset + 2, dtype=torch.from_numpy(a[:0].copy()).dtype, device=Context.current().device)
    part = whole[offset:offset + a.size]
    part.copy_(torch.from_numpy(a.copy()))
    assert whole.data_ptr() % 16 == 0 and part.is_contiguous()
    return part


class Frame(object):
    """A case in device memory, its coordinate arrays `coord_offset` doubles into their allocations."""

    def __init__(self, case):
        from auromat_amd._native import Context
        from auromat_amd.util.histogram import make_axis
        self.case, self.ctx = case, Context.current()
        self.nch = case.img.shape[1]
        self.code = 2 if case.img.dtype == np.uint16 else 1
        co = case.coord_offset
        self.lat_c, self.lon_c = _device_array(case.lat_c, co), _device_array(case.lon_c, co)
        self.elev = None if case.elev is None else _device_array(case.elev, co)
        self.img = _device_array(case.img, co) if self.nch else None
        self.mask = None if case.mask is None else _device_array(case.mask.astype(np.uint8), co)
        self.cell_lat, self.cell_lon = _device_array(case.cell_lat, co), _device_array(case.cell_lon, co)
        assert self.lat_c.data_ptr() % 16 == 8 * co and self.cell_lon.data_ptr() % 16 == 8 * co
        self.xaxis, self._xkeep = make_axis(self.ctx, case.xedges, uniform=case.uniform)
        self.yaxis, self._ykeep = make_axis(self.ctx, case.yedges, uniform=case.uniform)
        assert self.xaxis.uniform == self.yaxis.uniform == int(case.uniform)

    def outputs(self):
        """Poisoned device outputs."""
        import torch
        ny, nx = self.case.shape
        out = dict(mesh=self.ctx.empty((ny, nx, self.nch + 1)),
                   img=self.ctx.empty((ny, nx, self.nch), torch.int16 if self.code == 2 else torch.uint8),
                   mask=self.ctx.empty((ny, nx), torch.uint8), triangle=self.ctx.empty((ny, nx), torch.int32))
        for t in out.values():
            t.view(torch.uint8).fill_(POISON)
        return out

    def claim_words(self, fill=0):
        """The caller's buffer for the claim words, dirty: zeros would make triangle 0 the winner of every cell if the call did
        not set the words itself."""
        import torch
        ny, nx = self.case.shape
        return torch.full((nx * ny,), fill, dtype=torch.int32, device=self.ctx.device)

    def enqueue(self, out, leave_out=(), claim=None):
        from auromat_amd._native import ptr
        case = self.case
        args = [ptr(out[k]) if (k not in leave_out and out[k].numel()) else None for k in OUT_KEYS]
        args.append(ptr(self.claim_words() if claim is None else claim))
        self.ctx.call('amt_mesh_frame', ptr(self.lat_c), ptr(self.lon_c), ptr(self.elev), ptr(self.img), self.code, self.nch,
                      ptr(self.mask), case.height, case.width, float(case.min_elevation), C.byref(self.xaxis), C.byref(self.yaxis),
                      case.lon_wrap, ptr(self.cell_lat), ptr(self.cell_lon), *args)

    def host(self, out):
        import torch
        torch.cuda.synchronize()
        got = {k: t.cpu().numpy() for k, t in out.items()}
        got['img'] = got['img'].view(self.case.img.dtype)
        return got

    def run(self, leave_out=(), claim=None):
        out = self.outputs()
        self.enqueue(out, leave_out, claim)
        return self.host(out)


def check_outputs(got, want, what, leave_out=()):
    for key in OUT_KEYS:
        if key in leave_out:
            assert (np.ascontiguousarray(got[key]).view(np.uint8) == POISON).all(), '%s: %s was written' % (what, key)
            continue
        bad = np.argwhere(~((got[key] == want[key]) | ((got[key] != got[key]) & (want[key] != want[key]))))
        assert O.same_bits(got[key], want[key]), '%s: %s differs in %d places, first %s: %r != %r' % (
            what, key, len(bad), tuple(bad[0]) if len(bad) else '(bits)', got[key][tuple(bad[0])] if len(bad) else None,
            want[key][tuple(bad[0])] if len(bad) else None)


_wanted = {}


def wanted(case):
    if case.name not in _wanted:
        _wanted[case.name] = O.mesh_frame(case)
    return _wanted[case.name]


@pytest.mark.parametrize('case', K.device_cases(), ids=repr)
def test_case_equals_oracle(case):
    check_outputs(Frame(case).run(), wanted(case), case.name)


@pytest.mark.parametrize('leave_out', OUT_KEYS)
def test_each_output_is_optional(leave_out):
    case = K.removal_cases()['masked']
    check_outputs(Frame(case).run(leave_out=(leave_out,)), wanted(case), '%s without %s' % (case.name, leave_out), (leave_out,))


def test_one_output_alone():
    case = K.wide_case()
    for key in OUT_KEYS:
        others = tuple(k for k in OUT_KEYS if k != key)
        check_outputs(Frame(case).run(leave_out=others), wanted(case), '%s, %s alone' % (case.name, key), others)


def test_the_claim_words_are_set_anew_by_every_call():
    """ONE buffer of claim words for a large grid full of claims, then a small one with few, then the large one again, on one
    context: no call sees the words of the one before; nor does it matter what the buffer held at first, and the call leaves
    the winners in it."""
    big, small = K.grid_cases()[4], K.grid_cases()[5]
    assert big.shape == (200, 200) and small.name == 'grid_coarse'
    claim = Frame(big).claim_words(fill=1)
    for case in (big, small, big, K.seam_case(), small):
        assert case.shape[0] * case.shape[1] <= claim.numel()
        check_outputs(Frame(case).run(claim=claim), wanted(case), case.name + ' (after another shape)')
    ny, nx = small.shape
    words = claim[:nx * ny].cpu().numpy().view(np.uint32).reshape(nx, ny)
    assert np.array_equal(words, O.claims(small))
    for fill in (-1, 0x5A5A5A5A):
        check_outputs(Frame(small).run(claim=Frame(small).claim_words(fill)), wanted(small), 'claim words filled with %x' % fill)


def test_two_runs_give_the_same_bits():
    frame = Frame(K.dyadic_case())
    a, b = frame.run(), frame.run()
    for key in OUT_KEYS:
        assert a[key].tobytes() == b[key].tobytes(), key


def test_on_a_side_stream_behind_a_gate():
    """The call on a side stream whose inputs arrive behind a gate (tests/_gated_stream.py): it only enqueues, on the stream
    the context follows.  The decoy is another lattice over the same grid: finite coordinates, no input is used as an index."""
    import _gated_stream as G
    from auromat_amd._native import ptr
    from auromat_amd.util.histogram import make_axis
    true = K.shape_cases()[4]
    h, w = true.lat_c.shape
    dx, dy = K.lattice_xy(h, w, 3.0, 4.0, 0.7, 0.4, jitter=0.1, seed=99)
    rng = np.random.RandomState(98)
    inputs = [('lat_c', (true.lat_c, dy)), ('lon_c', (true.lon_c, dx)), ('elev', (true.elev, rng.uniform(0, 90, (h, w)))),
              ('img', (true.img, rng.randint(0, 256, true.img.shape).astype(np.uint8)))]
    ny, nx = true.shape
    outputs = [('mesh', ((ny, nx, 4), np.float64)), ('img_out', ((ny, nx, 3), np.uint8)), ('mask', ((ny, nx), np.uint8)),
               ('triangle', ((ny, nx), np.int32))]
    keep = {}

    def call(env):
        if 'axes' not in keep:
            keep['axes'] = (make_axis(env.ctx, true.xedges, uniform=True), make_axis(env.ctx, true.yedges, uniform=True))
            keep['cells'] = (G.dev(true.cell_lat), G.dev(true.cell_lon))
            keep['claim'] = G.dev(np.zeros(nx * ny, dtype=np.int32))
        (xaxis, _), (yaxis, _) = keep['axes']
        env.ctx.call('amt_mesh_frame', ptr(env.inp['lat_c']), ptr(env.inp['lon_c']), ptr(env.inp['elev']), ptr(env.inp['img']), 1, 3,
                     None, h, w, float('-inf'), C.byref(xaxis), C.byref(yaxis), 0, ptr(keep['cells'][0]), ptr(keep['cells'][1]),
                     ptr(env.out['mesh']), ptr(env.out['img_out']), ptr(env.out['mask']), ptr(env.out['triangle']), ptr(keep['claim']))
        env.closed('amt_mesh_frame')

    case = G.Case('mesh_cells_gated', 'A', inputs, outputs, call,
                  harmless='coordinates and values only; cell indices are clamped to the grid, claim words come from the call itself')
    G.run_gated(case)
    want = wanted(true)
    got, _, _ = G.baseline(case)
    assert O.same_bits(got['mesh'].view(np.float64).reshape(ny, nx, 4), want['mesh'])
    assert np.array_equal(got['triangle'].view(np.int32).reshape(ny, nx), want['triangle'])


def test_bad_arguments_are_refused():
    from auromat_amd._native import NativeError, ptr
    frame = Frame(K.removal_cases()['whole'])
    out = frame.outputs()
    case = frame.case

    claim = frame.claim_words()

    def call(height=case.height, width=case.width, nch=frame.nch, code=1, outs=None, lat_c=frame.lat_c, cells=frame.cell_lat,
             words=claim):
        outs = [ptr(out[k]) for k in OUT_KEYS] if outs is None else outs
        frame.ctx.call('amt_mesh_frame', ptr(lat_c), ptr(frame.lon_c), ptr(frame.elev), ptr(frame.img), code, nch, None, height, width,
                       float('-inf'), C.byref(frame.xaxis), C.byref(frame.yaxis), 0, ptr(cells), ptr(frame.cell_lon),
                       *(outs + [ptr(words)]))

    call()
    for kw in (dict(height=1), dict(width=1), dict(height=0), dict(nch=5), dict(nch=-1), dict(code=3), dict(outs=[None] * 4),
               dict(lat_c=None), dict(cells=None), dict(words=None), dict(height=2, width=1 << 30), dict(height=32769, width=32769)):
        with pytest.raises(NativeError):
            call(**kw)
    # (nothing was enqueued by the refused calls: the outputs of the one good call stand)
    check_outputs(frame.host(out), wanted(case), 'after refused calls')
