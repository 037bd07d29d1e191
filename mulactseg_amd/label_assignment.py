"""The data-generation step of the reference: multi-hot query labels and dominant-label maps for a whole datalist, on the GPU.

    python -m mulactseg_amd.label_assignment multi_hot --nseg 2048 --trim_multihot_boundary --trim_kernel_size 5 --save_data_dir DIR
    python -m mulactseg_amd.label_assignment dominant --nseg 2048 --generate_ignore --loader region_cityscapes_dominant_all_sample

replace ``tools/label_assignment_tensor[_voc].py`` (``multi_hot_cls.npy`` u8 ``[N_img, nseg, C+1]`` and ``sp_size.npy`` int64
``[N_img, nseg]``, rows in datalist order; logic ``dataloader/region_cityscapes_tensor.py:23-86``) and
``tools/label_assignment_dominant[_voc].py`` (16-bit grayscale PNGs under ``gtFine_dominant[_ignore][_sample]`` and colour PNGs under
``gtColor_dominant...``; logic ``dataloader/region_cityscapes_dominant_all[_sample].py:24-62``).  The flags are the reference tools'
under their names and defaults; ``--dataset voc`` gives the VOC tools' defaults, ``--trg_datalist`` / ``--region_dict`` override the
reference's relative defaults, ``--seed`` seeds the ``_sample`` draw.

Per picture: host threads decode the label and superpixel files (``picture_store.decode_map``), one upload, the kernels of
``csrc/labels.hip`` on the stream, one copy back (the 40 KB multi-hot row of a Cityscapes picture, or the dominant map), PNG encoding
on the same threads.  The ``.npy`` files are written once at the end, through a temporary name and a rename.

The ``_sample`` variant draws ``torch.multinomial(torch.Tensor(counts), 1)`` on the host, in the reference's call order (pictures in
datalist order, ids in region-dict order) from a ``torch.Generator`` seeded with ``--seed``, after the one draw with which the
reference's DataLoader iterator takes its base seed.  That equals the reference at ``--num_worker 0`` after
``torch.manual_seed(seed)`` under the same torch; the reference itself does not reproduce across torch versions or worker counts.
"""
import argparse
import concurrent.futures
import os
import sys
import time

import numpy as np
import torch

from . import ops
from .dataloader import constant, formats, region_voc
from .dataloader.picture_store import decode_map

IGNORE = 255
_VOC_SEEDS_DIR = {150: 32, 600: 16}           # the directories region_voc_or_tensor.py reads the multi-hot tensors from


# ------------------------------------------------------------------------------------------------
# one picture
# ------------------------------------------------------------------------------------------------
def multinomial_draw(full, ids, num_classes, generate_ignore, generator):
    """int32 [nseg]: the column ``region_cityscapes_dominant_all_sample.py:41-49`` draws for each listed id (-1: no pixel counted),
    consuming ``generator`` exactly as the reference's loop consumes the global generator: one ``torch.multinomial`` per listed id
    in list order whose histogram is not empty -- a repeated id draws again over the already painted region (one value)."""
    full = np.asarray(full)
    hi = num_classes + 1 if generate_ignore else num_classes
    drawn = np.full(full.shape[0], -1, dtype=np.int32)
    done = set()
    for p in ids:
        p = int(p)
        row = full[p, :hi].astype(np.int64)
        if p in done:                                    # the region already holds its drawn value: u = [value], c = [n]
            n = int(row.sum())
            if n:
                torch.multinomial(torch.Tensor(np.array([n])), num_samples=1, replacement=False, generator=generator)
            continue
        done.add(p)
        nz = np.nonzero(row)[0]
        if nz.size:
            i = torch.multinomial(torch.Tensor(row[nz]), num_samples=1, replacement=False, generator=generator).item()
            drawn[p] = nz[i]
    return drawn


def sample_generator(seed):
    """The generator of the ``_sample`` replay: seeded, then advanced by the base-seed draw of the reference's DataLoader iterator
    (``iter(DataLoader)`` takes ``torch.empty((), dtype=torch.int64).random_()`` before the first picture)."""
    g = torch.Generator()
    g.manual_seed(int(seed))
    torch.empty((), dtype=torch.int64).random_(generator=g)
    return g


def _as_device(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def assign(labels, superpixel, ids, nseg, num_classes, trim_kernel_size=None, dominant=False, generate_ignore=False, generator=None,
           device='cuda'):
    """The label assignment of one picture on the GPU.  labels: train ids [H,W] (uint8, or any integer type holding values in
    [0, num_classes) and 255); superpixel: ids [H,W] (int64 / int32 / int16 / uint16); ids: the region dict's list for the picture.

    Multi-hot (``dominant=False``): ``(cls uint8 [nseg, num_classes + 1], size int64 [nseg])`` as numpy arrays.
    Dominant: the dominant-label map, numpy uint8 [H,W]; ``generator`` (a ``torch.Generator``) selects the ``_sample`` draw."""
    lab = labels.cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if lab.dtype != np.uint8:
        if lab.size and (lab.min() < 0 or lab.max() > IGNORE):
            raise ValueError("label values must be in [0, %d) or %d" % (num_classes, IGNORE))
        lab = lab.astype(np.uint8)
    spx = superpixel.cpu().numpy() if torch.is_tensor(superpixel) else np.asarray(superpixel)
    if spx.dtype not in (np.int64, np.int32, np.int16, np.uint16):
        spx = spx.astype(np.int64)
    lab_d, spx_d = _as_device(lab, device), _as_device(spx, device)
    if not dominant:
        bits, size = ops.region_multi_hot(lab_d, spx_d, ids, nseg, num_classes, trim_kernel_size)
        return bits.cpu().numpy(), size.cpu().numpy()
    draw = None
    if generator is not None:
        def draw(full):
            return multinomial_draw(full, ids, num_classes, generate_ignore, generator)
    return ops.region_dominant(lab_d, spx_d, ids, nseg, num_classes, generate_ignore, draw).cpu().numpy()


# ------------------------------------------------------------------------------------------------
# the command line
# ------------------------------------------------------------------------------------------------
_DEFAULTS = {
    'cityscapes': dict(nseg=2048, num_classes=19, trg_data_dir='./data/Cityscapes'),
    'voc': dict(nseg=150, num_classes=21, trg_data_dir='./data/VOCdevkit'),
}


def get_parser():
    p = argparse.ArgumentParser(prog='python -m mulactseg_amd.label_assignment',
                                description='multi-hot query labels / dominant-label maps of a datalist (GPU)')
    sub = p.add_subparsers(dest='mode', required=True)
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument('--dataset', choices=('cityscapes', 'voc'), default='cityscapes')
    common.add_argument('--nseg', type=int, default=None, help='superpixels per picture (2048; voc 150)')
    common.add_argument('--num_classes', type=int, default=None, help='classes of the dataset (19; voc 21)')
    common.add_argument('--num_worker', type=int, default=8, help='decode / encode threads')
    common.add_argument('--trg_data_dir', default=None, help='data root (./data/Cityscapes; voc ./data/VOCdevkit)')
    common.add_argument('--spx_method', default='seed')
    common.add_argument('--trg_datalist', default=None, help="datalist (the reference's dataloader/init_data/... path by default)")
    common.add_argument('--region_dict', default=None, help="region dict (the reference's dataloader/init_data/... path by default)")
    common.add_argument('--seed', type=int, default=0, help='seed of the _sample draw')
    m = sub.add_parser('multi_hot', parents=[common], help='multi_hot_cls.npy + sp_size.npy (tools/label_assignment_tensor.py)')
    m.add_argument('--save_data_dir', default=None, help='output directory (default: where the multi-hot loaders read)')
    m.add_argument('--trim_kernel_size', type=int, default=3)
    m.add_argument('--trim_multihot_boundary', action='store_true', default=False)
    m.add_argument('--ignore_size', type=int, default=0, help='parsed; changes nothing (as in the reference)')
    m.add_argument('--mark_topk', type=int, default=-1, help='parsed; changes nothing (as in the reference)')
    m.add_argument('--prob_dominant', action='store_true', default=False, help='parsed; changes nothing (as in the reference)')
    d = sub.add_parser('dominant', parents=[common], help='gtFine_dominant* PNGs (tools/label_assignment_dominant.py)')
    d.add_argument('--generate_ignore', action='store_true', default=False)
    d.add_argument('--loader', default='region_cityscapes_dominant_all',
                   help="a name containing 'sample' selects the _sample variant (region_cityscapes_dominant_all_sample)")
    d.add_argument('--nvis_color', type=int, default=3000, help='colour PNGs for the first N pictures')
    return p


def resolve(args):
    """Fill the dataset defaults and the derived paths in ``args`` (returned)."""
    for k, v in _DEFAULTS[args.dataset].items():
        if getattr(args, k) is None:
            setattr(args, k, v)
    voc = args.dataset == 'voc'
    if args.trg_datalist is None:
        args.trg_datalist = ('dataloader/init_data/voc/train_seed{}.txt'.format(args.nseg) if voc else
                             'dataloader/init_data/cityscapes/train_{}{}.txt'.format(args.spx_method, args.nseg))
    if args.region_dict is None:
        args.region_dict = ('dataloader/init_data/voc/train_seed{}.dict'.format(args.nseg) if voc else
                            'dataloader/init_data/cityscapes/train_{}{}.dict'.format(args.spx_method, args.nseg))
    if args.mode == 'multi_hot':
        args.trim = ops.trim_kernel(args.trim_kernel_size) if args.trim_multihot_boundary else 0
        if args.save_data_dir is None:
            args.save_data_dir = default_save_dir(args)
        args.known_ignore = False
        args.sample = False
    else:
        args.trim = 0
        args.known_ignore = not args.generate_ignore
        args.sample = 'sample' in args.loader
        args.do_data_dir = dominant_dir(args)
    return args


def default_save_dir(args):
    """Where RegionCityscapesOr / RegionVOCOr read the tensors (the reference's tool has no default and fails without the flag)."""
    name = "gtFine_multi_tensor_trim_{0}x{0}".format(args.trim) if args.trim else None
    if args.dataset == 'voc':
        if args.nseg not in _VOC_SEEDS_DIR:
            raise SystemExit("--save_data_dir is required for VOC with --nseg other than 150 / 600")
        return '{}/superpixels/pascal_voc_seg/seeds_{}/train/{}'.format(args.trg_data_dir, _VOC_SEEDS_DIR[args.nseg], name or 'multihot')
    return os.path.dirname(formats.multi_hot_paths(args.trg_data_dir, args.spx_method, args.nseg, args.trim or None)[0])


def dominant_dir(args):
    """``args.do_data_dir`` of tools/label_assignment_dominant[_voc].py (rooted at --trg_data_dir, which the reference hard-codes to
    its default)."""
    if args.dataset == 'voc':
        base = '{}/superpixels/pascal_voc_seg/seeds_{}/train/gtFine_dominant'.format(args.trg_data_dir, args.nseg)
    else:
        base = '{}/superpixel_seed/cityscapes/{}_{}/train/gtFine_dominant'.format(args.trg_data_dir, args.spx_method, args.nseg)
    if args.generate_ignore:
        base += '_ignore'
    if args.sample:
        base += '_sample'
    return base


def dominant_file(args, img_path):
    """get_lbl_fname: the first three '_' fields of the picture's file name (VOC: without its 4-character extension)."""
    data_id = '_'.join(img_path.split('/')[-1].split('_')[:3])
    if args.dataset == 'voc':
        data_id = data_id[:-4]
    return '{}/{}.png'.format(args.do_data_dir, data_id)


def color_file(path):
    return path.replace("gtFine", "gtColor")


def read_pictures(args):
    """[(image, label, superpixel) paths], [listed ids] in datalist order."""
    if args.dataset == 'voc':
        ids = formats.load_region_dict(args.region_dict)
        with open(args.trg_datalist, 'r') as f:
            names = [line.split('\t')[0] for line in f.read().splitlines() if line]
        return [region_voc.voc_paths(args.trg_data_dir, n, False) for n in names], [ids[n] for n in names]
    im_idx, suppix = formats.read_datalist(args.trg_datalist, args.trg_data_dir, args.region_dict, known_ignore=args.known_ignore)
    return im_idx, [suppix[s] for _, _, s in im_idx]


def decode_pair(args, lbl_path, spx_path):
    """(labels uint8 [H,W] train ids, superpixel ids int16 / int32 [H,W]) -- encode_target of the dataset on the raw label map."""
    raw = decode_map(lbl_path)
    if raw.dtype != np.uint8:
        raise ValueError("%s: label values beyond 255" % lbl_path)
    lab = raw if args.dataset == 'voc' else constant.id_to_train_id_u8[raw]
    spx = decode_map(spx_path, allow_u8=False)
    if spx.shape != lab.shape:
        raise ValueError("%s and %s differ in shape" % (lbl_path, spx_path))
    return lab, spx


def decode_color(args, dom):
    t = dom.copy()
    if args.dataset == 'voc':
        t[dom == IGNORE] = 21
        return constant.voc_id_to_color_map[t]
    t[dom == IGNORE] = 19
    return constant.train_id_to_color[t].astype(np.uint8)


def write_dominant(args, path, dom, color):
    from PIL import Image
    # to_pil_image(int32) gives mode I, which PNG stores as 16-bit grayscale: the same file as a uint16 (I;16) image
    Image.fromarray(dom.astype(np.uint16)).save(path)
    if color:
        cpath = color_file(path)
        os.makedirs(os.path.dirname(cpath), exist_ok=True)
        Image.fromarray(np.ascontiguousarray(decode_color(args, dom), dtype=np.uint8)).save(cpath)


def _save_npy(path, arr):
    tmp = path + '.tmp'
    with open(tmp, 'wb') as f:
        np.save(f, arr)
    os.replace(tmp, path)


def run(args, device='cuda'):
    """The whole datalist; returns the summary dict it prints."""
    t0 = time.perf_counter()
    pictures, lists = read_pictures(args)
    n = len(pictures)
    C1 = args.num_classes + 1
    threads = max(1, int(args.num_worker))
    if args.mode == 'multi_hot':
        cls = np.zeros((n, args.nseg, C1), dtype=np.uint8)
        size = np.zeros((n, args.nseg), dtype=np.int64)
    else:
        os.makedirs(args.do_data_dir, exist_ok=True)
    gen = sample_generator(args.seed) if args.mode == 'dominant' and args.sample else None
    t_decode = t_gpu = t_write = 0.0
    stream = torch.cuda.Stream(device)
    with concurrent.futures.ThreadPoolExecutor(threads) as pool, torch.cuda.stream(stream):
        window = 2 * threads
        pending = {i: pool.submit(decode_pair, args, pictures[i][1], pictures[i][2]) for i in range(min(window, n))}
        writes = []
        for i in range(n):
            ta = time.perf_counter()
            lab, spx = pending.pop(i).result()
            if i + window < n:
                pending[i + window] = pool.submit(decode_pair, args, pictures[i + window][1], pictures[i + window][2])
            tb = time.perf_counter()
            lab_d, spx_d = torch.from_numpy(lab).to(device), torch.from_numpy(spx).to(device)
            if args.mode == 'multi_hot':
                bits, sz = ops.region_multi_hot(lab_d, spx_d, lists[i], args.nseg, args.num_classes, args.trim)
                cls[i] = bits.cpu().numpy()
                size[i] = sz.cpu().numpy()
                tc = time.perf_counter()
            else:
                draw = None
                if gen is not None:
                    def draw(full, ids=lists[i]):
                        return multinomial_draw(full, ids, args.num_classes, args.generate_ignore, gen)
                dom = ops.region_dominant(lab_d, spx_d, lists[i], args.nseg, args.num_classes, args.generate_ignore, draw).cpu().numpy()
                tc = time.perf_counter()
                writes.append(pool.submit(write_dominant, args, dominant_file(args, pictures[i][0]), dom, i < args.nvis_color))
                if len(writes) > window:
                    writes.pop(0).result()
            t_decode += tb - ta
            t_gpu += tc - tb
            t_write += time.perf_counter() - tc
        tw = time.perf_counter()
        for w in writes:
            w.result()
        t_write += time.perf_counter() - tw
    tw = time.perf_counter()
    if args.mode == 'multi_hot':
        os.makedirs(args.save_data_dir, exist_ok=True)
        _save_npy(os.path.join(args.save_data_dir, 'multi_hot_cls.npy'), cls)
        _save_npy(os.path.join(args.save_data_dir, 'sp_size.npy'), size)
    t_write += time.perf_counter() - tw
    out = {'mode': args.mode, 'pictures': n, 'seconds': round(time.perf_counter() - t0, 3), 'decode_wait_s': round(t_decode, 3),
           'gpu_s': round(t_gpu, 3), 'write_s': round(t_write, 3), 'threads': threads}
    print("label_assignment %s: %d pictures in %.2f s (decode wait %.2f s, GPU %.2f s, write %.2f s; %d threads)"
          % (args.mode, n, out['seconds'], t_decode, t_gpu, t_write, threads))
    return out


def main(argv=None):
    args = resolve(get_parser().parse_args(argv))
    if not torch.cuda.is_available():
        raise SystemExit("label_assignment needs a GPU (there is no CPU path)")
    run(args)


if __name__ == '__main__':
    sys.exit(main())
