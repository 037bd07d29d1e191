"""The similarity-weighted online pseudo labels on the GPU: the kernels of csrc/online_plbl.hip against the library's host loops through
csrc/online_plbl.h bit for bit -- labels, weight bits, soft-weight bits at the defined entries, live flags, both accumulators, the
int64 sums of dzq --, the modules against the executed reference (tests/golden/g16_simw_plbl.npz), ``forward_lowres`` against
``forward`` on materialised tensors, run-to-run identity, the empty case, refused arguments, and the two trainers end to end."""
import importlib
import logging
import tempfile
import types

import numpy as np
import pytest
import torch

import online_plbl_restated as R
from test_online_plbl_gpu import N_CLS, TH_, TS, TW_, _Train, _Val
from test_online_plbl_gpu import off_ratio_case, took_the_direct_path, uint16_edge_case
from test_simw_plbl_cpu import METHODS, _host_labels, _host_soft, golden, golden_inputs, negated_tensors, tensors

pytestmark = pytest.mark.gpu
TAUS = (0.1, 0.01)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mulactseg_amd import ops
    return ops


def _same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _bit_for_bit(ops, t, size, id_types=(torch.int64,)):
    invT = ops.inv_temperature(R.T)
    d = {k: v.cuda() for k, v in t.items()}
    grad = torch.tensor([16.0])
    # hard labels with the similarity as the weight, and the signed CE on them
    ref = _host_labels(t, size, weight_sim=True)
    for dt in id_types:
        labels, weight = ops.online_pseudo_labels(d['zq_p'], d['featq'], size, d['spx'].to(dt), d['msk'], targets=d['tgt'], invT=invT,
                                                  weight_sim=True)
        assert torch.equal(labels.cpu(), ref['labels']), dt
        assert _same_bits(weight, ref['weight']), dt
    for flags, th in ((ops.LCE_WEIGHTED | ops.LCE_SIGNED, 0.0), (ops.LCE_WEIGHTED, 0.0), (ops.LCE_THRESHOLD, 0.25)):
        r = ops.online_plbl_reference(None, None, size, None, None, zq=t['zq'], invT_ce=invT, mode=flags & 3, th=th,
                                      signed=bool(flags & ops.LCE_SIGNED), grad=grad, labels=ref['labels'], weight=ref['weight'])
        loss, acc = ops.label_ce_fwd_lowres(d['zq'], size, labels, weight, invT, flags, th)
        assert torch.equal(acc.cpu(), r['acc']) and _same_bits(loss, r['loss']), flags
        dzq, fix = ops.label_ce_bwd_lowres(d['zq'], size, labels, weight, acc, grad.cuda(), invT, flags, th, want_fix=True)
        assert torch.equal(fix.cpu(), r['dzq_fix']), flags
        assert torch.equal(dzq.cpu(), (r['dzq_fix'].double() * 2.0 ** -44).float())
    # soft weights and the soft CE
    counted = 0
    for tau in TAUS:
        r = _host_soft(t, size, tau, zq=t['zq'], grad=grad)
        defined = ~torch.isnan(r['softw'])
        for dt in id_types:
            spx = d['spx'].to(dt)
            softw, live, bits = ops.online_soft_weights(d['zq_p'], d['featq'], size, spx, d['msk'], targets=d['tgt'], invT=invT,
                                                        inv_tau=ops.inv_temperature(tau))
            assert torch.equal(live.cpu(), r['live']) and torch.equal(bits.cpu(), r['bits']), (tau, dt)
            assert _same_bits(softw.cpu()[defined], r['softw'][defined]), (tau, dt)
            mask = d['msk'].view(torch.uint8) if d['msk'].dtype == torch.bool else d['msk']
            loss, acc = ops.soft_ce_fwd_lowres(d['zq'], size, spx, mask, bits, softw, live, invT)
            assert torch.equal(acc.cpu(), r['acc']) and _same_bits(loss, r['loss']), (tau, dt)
            dzq, fix = ops.soft_ce_bwd_lowres(d['zq'], size, spx, mask, bits, softw, live, acc, grad.cuda(), invT, want_fix=True)
            assert torch.equal(fix.cpu(), r['dzq_fix']), (tau, dt)
            assert torch.equal(dzq.cpu(), (r['dzq_fix'].double() * 2.0 ** -44).float())
        counted = int(r['acc'][1])
    return int((ref['labels'] != 255).sum()), int((ref['weight'] < 0).sum()), counted


def test_kernels_equal_the_host_loops_on_the_golden_shape():
    ops = _gpu()
    labelled, negative, counted = _bit_for_bit(ops, golden_inputs(), (R.H, R.W), id_types=(torch.int64, torch.int32))
    assert labelled > 500 and negative >= 1 and counted == int(golden()['pwce_count'])


def test_kernels_equal_the_host_loops_on_the_edge_case():
    """37 x 45 from its quarter size; a picture without a selected pixel and one with selected one-hot pixels only (neither is live), a
    superpixel with all 20 bits, ids >= S outside the mask, two classes sharing a prototype pixel"""
    ops = _gpu()
    e = R.edge_case()
    labelled, negative, counted = _bit_for_bit(ops, tensors(e), e['size'], id_types=(torch.int64, torch.int32))
    assert labelled > 500 and negative >= 1 and counted == 2293


@pytest.mark.parametrize("c,ch,h,w,s", [(19, 64, 9, 300, 24), (7, 33, 21, 50, 12), (21, 256, 16, 24, 8)])
def test_kernels_equal_the_host_loops_on_other_paths(c, ch, h, w, s):
    """more than one tile across (W > 256), the generic class count (no LDS image in the backward), 19 and 21 classes, a picture whose
    sides are multiples of 4, other feature widths"""
    ops = _gpu()
    case = dict(zip(('zq_p', 'featq', 'zq', 'tgt', 'spx', 'msk'), R.inputs(31 + c, 2, c, ch, h, w, R.quarter(h), R.quarter(w), s, frac=0.6)))
    labelled, _, counted = _bit_for_bit(ops, tensors(case), (h, w))
    assert labelled > 0 and counted >= labelled


def test_kernels_equal_the_host_loops_with_uint16_ids():
    """the third instantiation of both per-pixel kernels and the uint16 read of the soft CE, never run by the other cases"""
    ops = _gpu()
    e, t = uint16_edge_case()
    labelled, negative, counted = _bit_for_bit(ops, t, e['size'], id_types=(torch.uint16,))
    assert labelled > 500 and negative >= 1 and counted == 2293


def test_kernels_equal_the_host_loops_off_the_x4_ratio():
    """``off_ratio_case``: the signed, weighted and threshold label CE and the soft CE at both temperatures"""
    ops = _gpu()
    t, size = off_ratio_case()
    labelled, _, counted = _bit_for_bit(ops, t, size)
    assert labelled > 0 and counted >= labelled
    # the soft CE once more, to see on the device's own output that the taps outside the image were there
    invT, d = ops.inv_temperature(R.T), {k: v.cuda() for k, v in t.items()}
    softw, live, bits = ops.online_soft_weights(d['zq_p'], d['featq'], size, d['spx'], d['msk'], targets=d['tgt'], invT=invT,
                                                inv_tau=ops.inv_temperature(TAUS[0]))
    mask = d['msk'].view(torch.uint8) if d['msk'].dtype == torch.bool else d['msk']
    _, acc = ops.soft_ce_fwd_lowres(d['zq'], size, d['spx'], mask, bits, softw, live, invT)
    _, fix = ops.soft_ce_bwd_lowres(d['zq'], size, d['spx'], mask, bits, softw, live, acc, torch.tensor([16.0]).cuda(), invT, want_fix=True)
    assert took_the_direct_path(acc.cpu(), fix.cpu())


def test_kernels_equal_the_host_loop_when_every_weight_off_the_prototypes_is_negative():
    ops = _gpu()
    case, t = negated_tensors()
    labelled, negative, _ = _bit_for_bit(ops, t, case['size'])
    assert negative == labelled - int(case['proto'].sum()) > 200


def _args(**kw):
    return types.SimpleNamespace(nseg=R.S, weight_wo_proto=False, th_wplbl=kw.get('th'), ce_temp=R.T, simw_temp=kw.get('tau', 0.1))


def _module(name, kw):
    from mulactseg_amd.utils import loss as L
    return getattr(L, name)(_args(**kw), R.S, R.T)


CLASSES = [('simw', 'LocalsimWProtoCE', {}, 'simw_abs'), ('simw_th', 'LocalsimWProtoCE', {'th': 0.25}, 'simw_th_abs'),
           ('pwce0', 'JointLocalProtoWeightingCE', {'tau': 0.1}, None), ('pwce1', 'JointLocalProtoWeightingCE', {'tau': 0.01}, None)]


@pytest.mark.parametrize("name,cls,kw,mass", CLASSES)
def test_modules_match_the_executed_reference(name, cls, kw, mass):
    """values within 2e-6 of the reference's (of the mass, for the sum that may cancel), gradients within 1e-4 of the largest of the
    reference's, pushed through the transpose of the bilinear upsampling; two runs give the same bytes"""
    _gpu()
    g = golden()
    assert float(g['th']) == 0.25 and tuple(g['taus']) == TAUS
    t = {k: v.cuda() for k, v in golden_inputs().items()}
    crit = _module(cls, kw)
    runs = []
    for _ in range(2):
        zt = t['zq'].clone().requires_grad_(True)
        loss = crit.forward_lowres(t['zq_p'], t['featq'], zt, (R.H, R.W), t['tgt'], t['spx'], t['msk'])
        loss.backward()
        runs.append((loss.detach(), zt.grad))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)) and torch.equal(runs[0][1], runs[1][1])
    if name.startswith('pwce'):
        k = int(name[-1])
        ref, want = float(g['pwce_loss'][k]), g['pwce_gradq'][k]
        scale = abs(ref)
    else:
        ref, want, scale = float(g[name + '_loss']), g[name + '_gradq'], float(g[mass])
    print("%s: %.7f against %.7f" % (name, float(runs[0][0]), ref))
    assert abs(float(runs[0][0]) - ref) <= 2e-6 * scale
    want = torch.from_numpy(want)
    err, top = float((runs[0][1].cpu() - want).abs().max()), float(want.abs().max())
    print("%s gradient: max error %.3e of max|ref| %.3e" % (name, err, top))
    assert top > 0 and err <= 1e-4 * top


@pytest.mark.parametrize("name,cls,kw,mass", CLASSES[:3])
def test_forward_lowres_equals_forward_on_materialised_tensors(name, cls, kw, mass):
    ops = _gpu()
    t = {k: v.cuda() for k, v in golden_inputs().items()}
    size = (R.H, R.W)
    crit = _module(cls, kw)
    low = crit.forward_lowres(t['zq_p'], t['featq'], t['zq'], size, t['tgt'], t['spx'], t['msk'])
    acc_low = crit.last_acc.clone()
    full = crit(ops.upsample_bilinear(t['zq_p'], size), ops.upsample_bilinear(t['featq'], size), ops.upsample_bilinear(t['zq'], size),
                t['tgt'], t['spx'], t['msk'])
    assert torch.equal(acc_low, crit.last_acc) and torch.equal(low.view(torch.int32), full.view(torch.int32)) and float(low) > 0


@pytest.mark.parametrize("cls", ['LocalsimWProtoCE', 'JointLocalProtoWeightingCE'])
def test_an_empty_mask_gives_zero_and_a_zero_gradient(cls):
    _gpu()
    t = {k: v.cuda() for k, v in golden_inputs().items()}
    zt = t['zq'].clone().requires_grad_(True)
    loss = _module(cls, {}).forward_lowres(t['zq_p'], t['featq'], zt, (R.H, R.W), t['tgt'], t['spx'], torch.zeros_like(t['msk']))
    loss.backward()
    assert float(loss) == 0.0 and float(zt.grad.abs().max()) == 0.0


def test_bad_arguments_launch_nothing():
    ops = _gpu()
    from mulactseg_amd import _lib
    t = {k: v.cuda() for k, v in golden_inputs().items()}
    invT, size = ops.inv_temperature(R.T), (R.H, R.W)
    with pytest.raises(_lib.MulActSegHipError):          # both weight flags at once
        ops.online_pseudo_labels(t['zq_p'], t['featq'], size, t['spx'], t['msk'], targets=t['tgt'], invT=invT, weight_wo_proto=True,
                                 weight_sim=True)
    with pytest.raises(_lib.MulActSegHipError):          # a feature width beyond MAS_OPL_MAX_FEAT
        ops.online_soft_weights(t['zq_p'], torch.zeros((R.N, 2049, R.HQ, R.WQ), device='cuda'), size, t['spx'], t['msk'], targets=t['tgt'],
                                invT=invT)
    with pytest.raises(_lib.MulActSegHipError):          # a temperature that is not positive
        ops.online_soft_weights(t['zq_p'], t['featq'], size, t['spx'], t['msk'], targets=t['tgt'], invT=invT, inv_tau=0.0)
    labels = torch.full((R.N, R.H, R.W), 255, dtype=torch.uint8, device='cuda')
    weight = torch.zeros((R.N, R.H, R.W), device='cuda')
    with pytest.raises(_lib.MulActSegHipError):          # the signed sum without the weighted mode
        ops.label_ce_fwd_lowres(t['zq'], size, labels, weight, invT, ops.LCE_THRESHOLD | ops.LCE_SIGNED)
    # a null softw, straight at the entry point: the wrapper always allocates one
    lib = _lib.load()
    bits = ops.target_bits(t['tgt'].to(torch.uint8).contiguous())
    mask = t['msk'].view(torch.uint8)
    live = torch.ones(R.N, dtype=torch.int32, device='cuda')
    acc = torch.full((2,), 7, dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    code = lib.mas_soft_ce_fwd_lowres(t['zq'].data_ptr(), R.HQ, R.WQ, t['spx'].data_ptr(), _lib.ID_I64, mask.data_ptr(), bits.data_ptr(), None,
                                      live.data_ptr(), R.N, R.C, R.H, R.W, R.S, invT, acc.data_ptr(), None, st)
    assert code != 0
    work = torch.empty(int(lib.mas_online_plbl_work_bytes(R.N, R.S, R.C)) // 8, dtype=torch.int64, device='cuda')
    code = lib.mas_online_soft_weights(t['zq_p'].data_ptr(), t['featq'].data_ptr(), R.CH, R.HQ, R.WQ, t['spx'].data_ptr(), _lib.ID_I64,
                                       mask.data_ptr(), bits.data_ptr(), R.N, R.C, R.H, R.W, R.S, invT, 10.0, work.data_ptr(),
                                       work.numel() * 8, None, live.data_ptr(), st)
    assert code != 0
    torch.cuda.synchronize()
    assert acc.tolist() == [7, 7] and live.tolist() == [1] * R.N                # neither call touched its outputs


@pytest.mark.parametrize("method", METHODS)
def test_trainers_run_two_steps(method):
    """two steps at 128 x 160, S = 64, batch 2: finite losses, moving parameters, the reference's meters, the module in training mode
    after each pseudo-label forward, the quarter-resolution path taken"""
    _gpu()
    from mulactseg_amd import dataloader
    from mulactseg_amd.utils import common, loss as L
    simw = method == METHODS[0]
    extra = ['--dorampup', '--lamscale', '2.0'] if simw else ['--simw_temp', '0.05', '--simw_temp_schedule']
    a = common.get_parser().parse_args([
        '-m', 'deeplabv3pluswn_resnet50deepstem', '--separable_conv', '--method', method, '--ce_temp', '0.1', '--multi_ce_temp', '0.1',
        '--group_ce_temp', '0.1', '--coeff', '16.0', '--or_labeling', '--fair_counting', '--nseg', str(TS), '--train_batch_size', '2',
        '--val_batch_size', '1', '--num_workers', '0', '--val_num_workers', '0', '--train_lr', '2e-4', '--finetune_itrs', '2',
        '--val_period', '1000', '--log_period', '1', '-p', tempfile.mkdtemp()] + extra)
    a.pretrained_backbone = False
    dataloader.register_dataset_factory(lambda args, name, data_root, datalist, imageset: _Val())
    torch.manual_seed(0)
    tr = importlib.import_module("mulactseg_amd.trainer." + method).ActiveTrainer(a, logging.getLogger("test"), 1)
    crit = tr.multi_local_proto_loss if simw else tr.joint_local_proto_weight_loss
    assert isinstance(crit, L.LocalsimWProtoCE if simw else L.JointLocalProtoWeightingCE)
    seen = dict(plbl=[], meters=[], lowres=[], taus=[])
    plf, meter, fwd, low = tr.pseudo_label_forward, tr.update_average_meter, tr.forward_train, crit.forward_lowres

    def pseudo_label_forward(images, lowres):
        feats, logits = plf(images, lowres)
        assert tr.net.training and not logits.requires_grad          # restored after the eval-mode forward
        seen['plbl'].append((tuple(logits.shape), lowres))
        return feats, logits

    def update_average_meter(values):
        seen['meters'].append({k: v.detach().clone() for k, v in values.items()})
        return meter(values)

    def forward_train(images, **kw):
        seen['lowres'].append(kw.get('lowres', False))
        return fwd(images, **kw)

    def forward_lowres(*args, **kw):
        seen['taus'].append(kw.get('simw_temp'))
        return low(*args, **kw)

    tr.pseudo_label_forward, tr.update_average_meter, tr.forward_train = pseudo_label_forward, update_average_meter, forward_train
    crit.forward_lowres = forward_lowres
    tr._wandb_log = lambda payload, step: None
    before = [p.detach().clone() for p in tr.net.parameters()]
    tr.train(types.SimpleNamespace(selection_iter=1, get_trainset=lambda: _Train()))
    assert seen['plbl'] == [((2, N_CLS + 1, TH_ // 4, TW_ // 4), True)] * 2 and seen['lowres'] == [True, True]
    want = {'train-loss', 'pos-loss', 'local-proto-loss'} if simw else {'train-loss'}
    for m in seen['meters']:
        assert set(m) == want and all(bool(torch.isfinite(v)) for v in m.values())
    assert len(seen['meters']) == 2 and len(seen['taus']) == 2
    moved = sum(float((p.detach() - q).abs().sum()) for p, q in zip(tr.net.parameters(), before))
    assert moved > 0 and np.isfinite(moved) and tr.net.training
    first = seen['meters'][0]
    if simw:                        # lambda of step 0 is ramp_up(0) = 0: the first train-loss is coeff * pos
        assert float(first['pos-loss']) > 0 and float(first['local-proto-loss']) != 0
        assert abs(float(first['train-loss']) - 16.0 * float(first['pos-loss'])) <= 1e-5 * abs(float(first['train-loss']))
    else:                           # the schedule holds the temperature at 1000 and leaves args alone
        assert seen['taus'] == [1000.0, 1000.0] and a.simw_temp == 0.05 and float(first['train-loss']) > 0
