"""``k_within_eval`` (csrc/within_eval.hip) on the GPU: bit for bit against the library's host statement (labels, counters, diagnostics)
on the golden shape, the edge case, class counts with and without a build of their own, uint16 ids and a geometry off the x4 ratio;
accumulation; refusals that launch nothing; the fused path against the ``MAS_WITHIN_EVAL=aten`` chain; the allocator peak; and the four
trainers end to end over a small labelled set."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import online_plbl_restated as O
import within_eval_restated as R
from mulactseg_amd import synth

pytestmark = pytest.mark.gpu
METHODS = ('eval_cosplbl_within_multihot', 'eval_cosplbl_filt_within_multihot', 'eval_maxcosplbl_within_multihot',
           'eval_ensemble_plbl_within_multihot')


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def random_case(seed, C, Ch, h, w, H, W, S, N=2, ids=np.int64):
    """(zq, featq, targets, spx, mask, gt, (H, W)): half of the pixels' superpixels selected, rows of 1-4 classes, a few rows emptied
    and a few selected ids pushed out of range, so that every branch of the validity rule is taken"""
    rs = np.random.RandomState(seed)
    zq = synth.logits(seed, N, C, h, w)
    featq = F.normalize(torch.from_numpy(rs.standard_normal((N, Ch, h, w)).astype(np.float32)), dim=1).numpy()
    spx = np.stack([synth.superpixel_map(seed * 3 + i, H, W, S) for i in range(N)])
    tgt = np.stack([synth.multi_hot_targets(seed * 5 + i, S, C, p_counts=(0.4, 0.35, 0.15, 0.1)) for i in range(N)])
    chosen = rs.uniform(size=(N, S)) < 0.5
    msk = np.take_along_axis(chosen, spx.reshape(N, -1), axis=1).reshape(N, H, W)
    tgt[:, 0] = 0
    msk |= spx == 0                                                              # a selected superpixel with an empty row
    stray = msk & (rs.uniform(size=msk.shape) < 0.01)
    spx = np.where(stray, S + 3, spx)
    gt = R.ground_truth(seed, N, C - 1, H, W)
    return zq, featq, tgt, spx.astype(ids), msk, gt, (H, W)


def case(name):
    if name == 'golden':
        return R.inputs() + ((R.H, R.W),)
    if name == 'edge':
        e = R.edge_case()
        return tuple(e[k] for k in ('zq_p', 'featq', 'tgt', 'spx', 'msk', 'gt')) + (e['size'],)
    if name == 'u16':
        return random_case(31, 20, 48, 12, 20, 48, 80, 30, ids=np.uint16)
    if name == 'off_ratio':                                                      # x3.4 down, x2.6 across: no tap of the x4 pattern
        return random_case(32, 20, 40, 10, 25, 34, 65, 20, ids=np.int32)
    C, Ch, h, w, S = name
    return random_case(33 + C, C, Ch, h, w, 4 * h, 4 * w, S)


CASES = ['golden', 'edge', (19, 64, 9, 300, 24), (7, 33, 21, 50, 12), (21, 256, 16, 24, 8), 'u16', 'off_ratio']


@pytest.fixture(scope="module")
def host_statement():
    """the host statement of every case and mode, computed once"""
    from mulactseg_amd import ops
    cache = {}

    def get(name, mode):
        if (name, mode) not in cache:
            zq, featq, tgt, spx, msk, gt, size = case(name)
            spx_t = t(spx.astype(np.int32)).to(torch.uint16) if spx.dtype == np.uint16 else t(spx)
            cache[(name, mode)] = ops.within_multihot_reference(t(zq), t(featq), size, spx_t, t(msk), t(gt), targets=t(tgt), mode=mode)
        return cache[(name, mode)]
    return get


def device_inputs(name):
    zq, featq, tgt, spx, msk, gt, size = case(name)
    spx_t = t(spx.astype(np.int32)).to(torch.uint16) if spx.dtype == np.uint16 else t(spx)
    return [a.cuda() for a in (t(zq), t(featq), t(tgt), spx_t, t(msk), t(gt))], size


@pytest.mark.parametrize("mode", ['proto', 'filt'])
@pytest.mark.parametrize("name", CASES, ids=str)
def test_kernel_equals_the_host_statement_bit_for_bit(host_statement, name, mode):
    ops = _gpu()
    want = host_statement(name, mode)
    (zq, featq, tgt, spx, msk, gt), size = device_inputs(name)
    bits = ops.target_bits(tgt)
    counts, diag, labels = ops.within_multihot_eval(zq, featq, size, spx, msk, gt, bits=bits, mode=mode, want_labels=True)
    assert labels.dtype == torch.uint8 and np.array_equal(labels.cpu().numpy(), want['labels'].numpy())
    assert np.array_equal(counts.cpu().numpy(), want['counts'].numpy()) and diag.tolist() == want['diag'].tolist()
    d = diag.tolist()
    print("%s %s: valid %d, prototypes %d, below %d, removed %d" % (name, mode, *d))
    assert d[0] > 0 and d[1] > 0 and (d[3] > 0) == (mode == 'filt')
    # without the label output, into the same counters: they double, and no map comes back
    c2, d2, none = ops.within_multihot_eval(zq, featq, size, spx, msk, gt, targets=tgt, mode=mode, counts=counts, diag=diag)
    assert none is None and c2 is counts and d2 is diag
    assert np.array_equal(counts.cpu().numpy(), 2 * want['counts'].numpy()) and diag.tolist() == [2 * v for v in want['diag'].tolist()]


def test_a_wider_meter_counts_the_same_map():
    ops = _gpu()
    (zq, featq, tgt, spx, msk, gt), size = device_inputs('golden')
    K = R.C + 5
    counts, _, labels = ops.within_multihot_eval(zq, featq, size, spx, msk, gt, targets=tgt, num_classes=K, want_labels=True)
    assert np.array_equal(counts.cpu().numpy(), R.counts(labels.cpu().numpy(), gt.cpu().numpy(), K))
    # and the same as the project's MeanIoU on that map
    from mulactseg_amd.utils.miou import MeanIoU
    meter = MeanIoU(K, R.IGNORE)
    meter._after_step({'outputs': labels.long(), 'targets': gt})
    assert torch.equal(meter._counts, counts)


def test_bad_arguments_launch_nothing():
    ops = _gpu()
    from mulactseg_amd import _lib
    lib = _lib.load()
    (zq, featq, tgt, spx, msk, gt), (H, W) = device_inputs('golden')
    bits, mask = ops.target_bits(tgt), msk.view(torch.uint8)
    N, C, h, w = zq.shape
    Ch, S = featq.shape[1], bits.shape[1]
    work = torch.empty(int(lib.mas_within_eval_work_bytes(N, S, C)) // 8, dtype=torch.int64, device='cuda')
    counts = torch.full((3 * C + 3,), 7, dtype=torch.int64, device='cuda')
    diag = torch.full((4,), 7, dtype=torch.int64, device='cuda')
    labels = torch.full((N, H, W), 7, dtype=torch.uint8, device='cuda')
    good = dict(zq=zq.data_ptr(), featq=featq.data_ptr(), Ch=Ch, h=h, w=w, spx=spx.data_ptr(), dt=_lib.ID_I64, mask=mask.data_ptr(),
                bits=bits.data_ptr(), N=N, C=C, H=H, W=W, S=S, gt=gt.data_ptr(), mode=0, K=C, ign=255, work=work.data_ptr(),
                wb=work.numel() * 8, counts=counts.data_ptr(), diag=diag.data_ptr(), labels=labels.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.mas_within_eval_counts(a['zq'], a['featq'], a['Ch'], a['h'], a['w'], a['spx'], a['dt'], a['mask'], a['bits'], a['N'], a['C'],
                                          a['H'], a['W'], a['S'], a['gt'], a['mode'], a['K'], a['ign'], a['work'], a['wb'], a['counts'],
                                          a['diag'], a['labels'], None)
    bad = [dict(zq=None), dict(featq=None), dict(gt=None), dict(counts=None), dict(diag=None), dict(work=None), dict(Ch=0),
           dict(Ch=_lib.MAX_CLASSES * 1000), dict(C=1), dict(C=33), dict(K=C - 1), dict(K=33), dict(mode=2), dict(mode=-1), dict(dt=7),
           dict(S=0), dict(h=H + 1), dict(wb=work.numel() * 8 - 8), dict(work=work.data_ptr() + 4), dict(counts=counts.data_ptr() + 4)]
    for kw in bad:
        status = call(**kw)
        torch.cuda.synchronize()
        assert status < 0, kw
        assert bool((counts == 7).all()) and bool((diag == 7).all()) and bool((labels == 7).all()), kw
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((labels[2] == 255).all()) and bool((labels[0] < C).any()) and int(diag[0]) > 7      # (picture 2 has nothing selected)
    with pytest.raises(ValueError, match="mode"):
        ops.within_multihot_eval(zq, featq, (H, W), spx, msk, gt, targets=tgt, mode='nearest')
    with pytest.raises(ValueError, match="num_classes"):
        ops.within_multihot_eval(zq, featq, (H, W), spx, msk, gt, targets=tgt, num_classes=C - 1)


@pytest.mark.parametrize("name,mode", [('eval_cosplbl_within_multihot', 'proto'), ('eval_cosplbl_filt_within_multihot', 'filt')])
def test_fused_path_equals_the_aten_chain_on_decided_pixels(name, mode):
    """the chain of MAS_WITHIN_EVAL=aten on the materialised upsampling of the same quarter-resolution maps; compared where the float64
    margin of the label exceeds 8 times the float32 error of a feature product, as for the golden"""
    ops = _gpu()
    (zq, featq, tgt, spx, msk, gt), size = device_inputs('golden')
    counts, diag, labels = ops.within_multihot_eval(zq, featq, size, spx, msk, gt, targets=tgt, mode=mode, want_labels=True)
    feats, logits = ops.upsample_bilinear(featq, size), ops.upsample_bilinear(zq, size)
    tr = object.__new__(importlib.import_module("mulactseg_amd.trainer." + name).ActiveTrainer)
    lab, below = tr.pseudo_label_generation(gt, feats, logits, tgt, msk, spx, with_below=True)
    r = R.generate(logits.cpu().numpy(), feats.cpu().numpy(), tgt.cpu().numpy(), spx.cpu().numpy(), msk.cpu().numpy(), mode)
    err = R.sim_err_f32(feats.cpu(), msk.cpu())
    decided = r['valid'] & (r['gap'] > 8 * err)
    skipped = int(r['valid'].sum() - decided.sum())
    print("%s: valid %d, near ties %d, sim_err %.3e, below fused %d aten %d" % (mode, r['valid'].sum(), skipped, err, int(diag[2]), int(below)))
    assert r['valid'].sum() >= 500 and 200 * skipped <= int(r['valid'].sum())
    got, chain = labels.cpu().numpy(), lab.cpu().numpy()
    assert np.array_equal(got[decided], chain[decided]) and np.all(chain[~r['valid']] == 255) and np.all(got[~r['valid']] == 255)
    assert r['below_margin'] > 8 * err and int(below) == int(diag[2]) == int(r['below'].sum())


def test_a_fused_call_allocates_less_than_the_full_resolution_logits():
    """the (21, 256, 16, 24, 8) shape scaled x4: the call's own allocations (work buffer, counters) stay far below one [N,C,H,W] tensor"""
    ops = _gpu()
    zq, featq, tgt, spx, msk, gt, (H, W) = random_case(54, 21, 256, 64, 96, 256, 384, 32)
    dev = [a.cuda() for a in (t(zq), t(featq), t(tgt), t(spx), t(msk), t(gt))]
    bits = ops.target_bits(dev[2])
    counts = torch.zeros(3 * 21 + 3, dtype=torch.int64, device='cuda')
    diag = torch.zeros(4, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ops.within_multihot_eval(dev[0], dev[1], (H, W), dev[3], dev[4], dev[5], bits=bits, counts=counts, diag=diag)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    full = 2 * 21 * H * W * 4
    print("allocator peak rises by %d bytes; one [N,C,H,W] f32 tensor is %d" % (rise, full))
    assert int(diag[0]) > 0 and rise < full


def test_the_four_trainers_run_end_to_end(tmp_path, capsys, monkeypatch):
    """one eval() each over a labelled set of two 256 x 512 pictures (the size at which this network's forward is the same from one call
    to the next, tests/test_candidate_plbl_gpu.py), from the same seeded weights"""
    _gpu()
    import helpers
    from mulactseg_amd import dataloader
    from test_naive_plbl_gpu import NSEG, _args, _generator, _selected_set
    H, W = 256, 512
    monkeypatch.delenv("MAS_WITHIN_EVAL", raising=False)
    tree = helpers.write_cityscapes_tree(str(tmp_path / 'data'), n=2, H=H, W=W, nseg=NSEG)
    run = tmp_path / 'run'
    ckpt = str(run / 'checkpoint01.tar')
    tables, outs = {}, {}
    datalist = None
    for method in METHODS:
        a = _args(tree, run, ['--init_checkpoint', ckpt, '--resume_checkpoint', ckpt, '--method', method, '--loader', 'eval_region_cityscapes_all',
                              '--train_transform', 'eval_spx'], or_labeling=True)
        datalist = datalist or _selected_set(a)
        gen = _generator(importlib.import_module('mulactseg_amd.trainer.' + method), a, ckpt)
        aset = dataloader.get_active_dataset(a, train_transform=a.train_transform)
        aset.trg_label_dataset.transform.target = (H, W)
        aset.selection_iter = 1
        aset.load_datalist(datalist)
        capsys.readouterr()
        with np.errstate(all='ignore'):
            tables[method] = gen.eval(aset, selection_iter=0)
        outs[method] = capsys.readouterr().out
        print(outs[method])
        cells = tables[method].split(',')
        assert len(cells) == 1 + 20 and all(c == '%.2f' % float(c) for c in cells if c not in ('nan', 'inf'))
    cos, filt, mx, ens = (outs[m] for m in METHODS)
    assert cos.count("[AL 0-round] IoU: evaluation") == 1 and "[AL 0-round] Precision: evaluation" in cos and "[AL 0-round] Recall: evaluation" in cos
    for o in (filt, mx, ens):
        assert o.count("[AL 0-round]: evaluation") == 1 and "Precision" not in o
    assert tables[METHODS[0]] == tables[METHODS[2]] == tables[METHODS[3]] and tables[METHODS[0]] in mx
    lines = mx.strip().splitlines()
    assert len(lines) >= 2 and all(l.strip().isdigit() for l in lines[:2]) and not lines[2].strip()           # one count per batch
    assert not any(l.strip().isdigit() for o in (cos, filt, ens) for l in o.splitlines())
