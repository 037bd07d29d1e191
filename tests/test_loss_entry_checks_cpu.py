"""The return code of every stage-1 scan entry point of csrc/losses.hip, and of the values / scales entry points, for each class of bad
input that is refused BEFORE anything is launched: a required pointer NULL, a forbidden flag combination or a flag of another family,
a class count of 1 or MAS_MAX_CLASSES + 1, an empty batch, a quarter-resolution plane larger than the full one or with one extent
missing, an unknown id type -- and pairs of them, where the order of the checks decides.  The codes are literals: what an entry point
answers is part of the ABI, and nothing else pins the order of the checks that the entry points share.  Pointers are addresses of
small host tensors; no call gets as far as reading one, so the file needs no GPU.  (The fused forward checks the id type only after its first launch: that
case is left out there, and the fused backward gets it at full resolution, where nothing precedes the scan.)"""
import pytest
import torch

from mulactseg_amd import _lib as L

CE, GROUP, TCE, RC, TOPONE = L.LOSS_CE, L.LOSS_GROUP, L.LOSS_TCE, L.LOSS_RC, L.LOSS_TOPONE
TOP1, ENT, WITHIN, WGROUP = L.LOSS_TOP1, L.LOSS_ENT, L.LOSS_WITHIN, L.LOSS_WGROUP
NULL, SHAPE, CLASSES, DTYPE, ALIGN, RANGE, WORKSPACE = -1, -2, -3, -4, -5, -6, -7         # MAS_ERR_* of csrc/common.h
N, C, H, W, S, LOW = 1, 4, 4, 8, 2, 2            # LOW: both extents of the quarter-resolution plane
_BUF = torch.zeros(64, dtype=torch.int64)       # every "pointer" is its address: never read, never written
PTR = _BUF.data_ptr()

_HEAD = "z spx dt mask bits"
_DIMS = "N C H W S invT flags"
# entry point -> (its arguments in the order of include/mulactseg_hip.h, flag family, pointers the base call requires)
ENTRIES = {
    "mas_partial_loss_fwd": ("%s %s gmax acc st" % (_HEAD, _DIMS), "plain", "z spx mask bits gmax acc"),
    "mas_partial_loss_bwd": ("%s gmax scale %s dz st" % (_HEAD, _DIMS), "plain", "z spx mask bits gmax scale dz"),
    "mas_partial_loss_fwd_lowres": ("z h w spx dt mask bits %s gmax acc st" % _DIMS, "plain", "z spx mask bits gmax acc"),
    "mas_partial_loss_bwd_lowres": ("z h w spx dt mask bits gmax scale %s fix st" % _DIMS, "plain", "z spx mask bits gmax scale fix"),
    "mas_partial_loss_fwd_fused": ("z h w spx dt mask targets cols_stored cols_used bits N C H W S invT flags weights work work_bytes "
                                   "losses st", "plain", "z spx mask work"),         # (`bits` is NULL in the base call)
    "mas_partial_loss_bwd_fused": ("z h w spx dt mask bits work grad weights %s dz fix st" % _DIMS, "plain", "z spx mask work grad dz fix"),
    "mas_teacher_loss_fwd": ("z zt h w spx dt mask bits N C H W S invT invT_x th flags gmax acc st", "teacher", "z zt spx mask bits gmax acc"),
    "mas_teacher_loss_bwd": ("z zt h w spx dt mask bits gmax scale N C H W S invT invT_x th flags dz fix st", "teacher",
                             "z zt spx mask bits gmax scale fix"),
    "mas_wgroup_loss_fwd": ("z zt h w spx dt mask bits %s gmax tmax acc losses st" % _DIMS, "wgroup", "z zt spx mask bits gmax tmax acc"),
    "mas_wgroup_loss_bwd": ("z zt h w spx dt mask bits gmax tmax scale %s dz fix st" % _DIMS, "wgroup",
                            "z zt spx mask bits gmax tmax scale fix"),
    "mas_loss_values": ("acc flags losses st", None, "acc losses"),
    "mas_loss_scales": ("acc grad flags scale st", None, "acc grad scale"),
    "mas_loss_values_weighted": ("acc flags weights losses st", None, "acc weights losses"),
    "mas_loss_scales_weighted": ("acc grad weights flags scale st", None, "acc grad weights scale"),
    "mas_teacher_loss_values": ("acc flags losses st", "teacher", "acc losses"),
    "mas_teacher_loss_scales": ("acc grad flags scale st", "teacher", "acc grad scale"),
}
BASE_FLAGS = {"plain": CE | GROUP, "teacher": CE | GROUP | TOP1, "wgroup": CE | GROUP | WGROUP, None: CE | GROUP}
BAD_FLAGS = {
    "plain": {"rc+topone": CE | RC | TOPONE, "rc without ce": GROUP | RC, "rc with tce": CE | TCE | RC, "topone with tce": CE | TCE | TOPONE,
              "top1": CE | TOP1, "ent": CE | ENT, "within": CE | WITHIN, "wgroup": CE | GROUP | WGROUP},
    "teacher": {"no fourth slot": CE | GROUP, "top1+ent": CE | TOP1 | ENT, "within with ent": CE | ENT | WITHIN, "rc": CE | TOP1 | RC,
                "tce": CE | TCE | TOP1, "wgroup": CE | GROUP | TOP1 | WGROUP},
    "wgroup": {"no group": CE | WGROUP, "no wgroup": CE | GROUP, "top1": CE | GROUP | WGROUP | TOP1, "rc": CE | GROUP | WGROUP | RC,
               "tce": CE | TCE | GROUP | WGROUP},
}
_INTS = {"dt": 0, "N": N, "C": C, "H": H, "W": W, "S": S, "h": LOW, "w": LOW, "cols_stored": C, "cols_used": C, "st": None}
_FLOATS = {"invT": 10.0, "invT_x": 10.0, "th": 0.5}


def _base(entry):
    names, family, _ = ENTRIES[entry]
    args = {}
    for name in names.split():
        args[name] = _INTS[name] if name in _INTS else _FLOATS.get(name, PTR)
    args["flags"] = BASE_FLAGS[family]
    if entry == "mas_partial_loss_fwd_fused":
        args["bits"] = None
        args["work_bytes"] = int(L.load().mas_partial_loss_work_bytes(N, S, C, args["flags"]))
        assert 0 < args["work_bytes"] <= _BUF.numel() * 8
    return args


def _cases(entry):
    """name -> the overrides of the base call.  Every case is refused before a launch: a case that were accepted would hand host
    addresses to a kernel, so none is generated on spec -- each kind below is one the entry point's own code checks first."""
    names, family, required = ENTRIES[entry]
    names = names.split()
    scan, low = "N" in names, "h" in names
    cases = {"%s NULL" % p: {p: None} for p in required.split()}
    for label, flags in (BAD_FLAGS.get(family, {}) if scan or family == "teacher" else {}).items():
        cases["flags: %s" % label] = {"flags": flags}
    if not scan:
        return cases
    cases.update({"C = 1": {"C": 1}, "C = 33": {"C": 33}, "N = 0": {"N": 0}})
    full = {"h": 0, "w": 0} if low else {}
    if entry != "mas_partial_loss_fwd_fused":
        cases["id type 7"] = dict(full, dt=7) if entry == "mas_partial_loss_bwd_fused" else {"dt": 7}
    if low:
        cases.update({"h > H": {"h": H + 1}, "w > W": {"w": W + 1}, "h > 0, w = 0": {"w": 0}})
        if "dz" in names and "dz" not in required.split():      # the teacher families' backward: dz instead of fix at full resolution
            cases["dz NULL at full resolution"] = dict(full, dz=None)
    if "invT_x" in names:
        cases.update({"invT_x = 0": {"invT_x": 0.0}, "invT_x NaN": {"invT_x": float("nan")}})
    if entry == "mas_partial_loss_fwd_fused":
        cases.update({"targets and bits NULL": {"targets": None}, "cols_used = 0": {"cols_used": 0},
                      "cols_used > cols_stored": {"cols_used": C + 1}, "work too small": {"work_bytes": 8},
                      "work misaligned": {"work": PTR + 4}})
    # two faults at once: the check that comes first in the entry point decides
    bad = next(iter(BAD_FLAGS[family].values()))
    cases.update({"z NULL and bad flags": {"z": None, "flags": bad}, "bad flags and N = 0": {"flags": bad, "N": 0},
                  "N = 0 and C = 1": {"N": 0, "C": 1}, "H = 0 and C = 33": {"H": 0, "C": 33}})
    if "dt" in names and entry != "mas_partial_loss_fwd_fused":
        cases["C = 1 and id type 7"] = dict(cases["id type 7"], C=1)
        cases["N = 0 and id type 7"] = dict(cases["id type 7"], N=0)
    if low:
        late = next(p for p in ("acc", "scale", "grad", "work") if p in names)
        cases.update({"C = 1 and h > H": {"C": 1, "h": H + 1}, "N = 0 and h > H": {"N": 0, "h": H + 1},
                      "bad flags and h > H": {"flags": bad, "h": H + 1},
                      "%s NULL and h > H" % late: {late: None, "h": H + 1}})
    if "zt" in names:
        cases.update({"zt and z NULL": {"zt": None, "z": None}, "zt NULL and bad flags": {"zt": None, "flags": bad},
                      "zt NULL and h > H": {"zt": None, "h": H + 1}})
    return cases


# what the library answers to every case (none of them 0: nothing is launched)
EXPECTED = {
    "mas_partial_loss_fwd": {
        "z NULL": NULL, "spx NULL": NULL, "mask NULL": NULL, "bits NULL": NULL, "gmax NULL": NULL, "acc NULL": NULL,
        "flags: rc+topone": RANGE, "flags: rc without ce": RANGE, "flags: rc with tce": RANGE, "flags: topone with tce": RANGE,
        "flags: top1": RANGE, "flags: ent": RANGE, "flags: within": RANGE, "flags: wgroup": RANGE, "C = 1": CLASSES, "C = 33": CLASSES,
        "N = 0": SHAPE, "id type 7": DTYPE, "z NULL and bad flags": NULL, "bad flags and N = 0": RANGE, "N = 0 and C = 1": SHAPE,
        "H = 0 and C = 33": SHAPE, "C = 1 and id type 7": CLASSES, "N = 0 and id type 7": SHAPE,
    },
    "mas_partial_loss_bwd": {
        "z NULL": NULL, "spx NULL": NULL, "mask NULL": NULL, "bits NULL": NULL, "gmax NULL": NULL, "scale NULL": NULL, "dz NULL": NULL,
        "flags: rc+topone": RANGE, "flags: rc without ce": RANGE, "flags: rc with tce": RANGE, "flags: topone with tce": RANGE,
        "flags: top1": RANGE, "flags: ent": RANGE, "flags: within": RANGE, "flags: wgroup": RANGE, "C = 1": CLASSES, "C = 33": CLASSES,
        "N = 0": SHAPE, "id type 7": DTYPE, "z NULL and bad flags": NULL, "bad flags and N = 0": RANGE, "N = 0 and C = 1": SHAPE,
        "H = 0 and C = 33": SHAPE, "C = 1 and id type 7": CLASSES, "N = 0 and id type 7": SHAPE,
    },
    "mas_partial_loss_fwd_lowres": {
        "z NULL": NULL, "spx NULL": NULL, "mask NULL": NULL, "bits NULL": NULL, "gmax NULL": NULL, "acc NULL": NULL,
        "flags: rc+topone": RANGE, "flags: rc without ce": RANGE, "flags: rc with tce": RANGE, "flags: topone with tce": RANGE,
        "flags: top1": RANGE, "flags: ent": RANGE, "flags: within": RANGE, "flags: wgroup": RANGE, "C = 1": CLASSES, "C = 33": CLASSES,
        "N = 0": SHAPE, "id type 7": DTYPE, "h > H": SHAPE, "w > W": SHAPE, "h > 0, w = 0": SHAPE, "z NULL and bad flags": NULL,
        "bad flags and N = 0": RANGE, "N = 0 and C = 1": SHAPE, "H = 0 and C = 33": SHAPE, "C = 1 and id type 7": CLASSES,
        "N = 0 and id type 7": SHAPE, "C = 1 and h > H": SHAPE, "N = 0 and h > H": SHAPE, "bad flags and h > H": SHAPE,
        "acc NULL and h > H": NULL,
    },
    "mas_partial_loss_bwd_lowres": {
        "z NULL": NULL, "spx NULL": NULL, "mask NULL": NULL, "bits NULL": NULL, "gmax NULL": NULL, "scale NULL": NULL, "fix NULL": NULL,
        "flags: rc+topone": RANGE, "flags: rc without ce": RANGE, "flags: rc with tce": RANGE, "flags: topone with tce": RANGE,
        "flags: top1": RANGE, "flags: ent": RANGE, "flags: within": RANGE, "flags: wgroup": RANGE, "C = 1": CLASSES, "C = 33": CLASSES,
        "N = 0": SHAPE, "id type 7": DTYPE, "h > H": SHAPE, "w > W": SHAPE, "h > 0, w = 0": SHAPE, "z NULL and bad flags": NULL,
        "bad flags and N = 0": RANGE, "N = 0 and C = 1": SHAPE, "H = 0 and C = 33": SHAPE, "C = 1 and id type 7": CLASSES,
        "N = 0 and id type 7": SHAPE, "C = 1 and h > H": SHAPE, "N = 0 and h > H": SHAPE, "bad flags and h > H": SHAPE,
        "scale NULL and h > H": NULL,
    },
    "mas_partial_loss_fwd_fused": {
        "z NULL": NULL, "spx NULL": NULL, "mask NULL": NULL, "work NULL": NULL, "flags: rc+topone": RANGE, "flags: rc without ce": RANGE,
        "flags: rc with tce": RANGE, "flags: topone with tce": RANGE, "flags: top1": RANGE, "flags: ent": RANGE, "flags: within": RANGE,
        "flags: wgroup": RANGE, "C = 1": CLASSES, "C = 33": CLASSES, "N = 0": SHAPE, "h > H": SHAPE, "w > W": SHAPE,
        "h > 0, w = 0": SHAPE, "targets and bits NULL": NULL, "cols_used = 0": CLASSES, "cols_used > cols_stored": CLASSES,
        "work too small": WORKSPACE, "work misaligned": ALIGN, "z NULL and bad flags": NULL, "bad flags and N = 0": RANGE,
        "N = 0 and C = 1": SHAPE, "H = 0 and C = 33": SHAPE, "C = 1 and h > H": CLASSES, "N = 0 and h > H": SHAPE,
        "bad flags and h > H": RANGE, "work NULL and h > H": NULL,
    },
    "mas_partial_loss_bwd_fused": {
        "z NULL": NULL, "spx NULL": NULL, "mask NULL": NULL, "work NULL": NULL, "grad NULL": NULL, "dz NULL": NULL, "fix NULL": NULL,
        "flags: rc+topone": RANGE, "flags: rc without ce": RANGE, "flags: rc with tce": RANGE, "flags: topone with tce": RANGE,
        "flags: top1": RANGE, "flags: ent": RANGE, "flags: within": RANGE, "flags: wgroup": RANGE, "C = 1": CLASSES, "C = 33": CLASSES,
        "N = 0": SHAPE, "id type 7": DTYPE, "h > H": SHAPE, "w > W": SHAPE, "h > 0, w = 0": SHAPE, "z NULL and bad flags": NULL,
        "bad flags and N = 0": RANGE, "N = 0 and C = 1": SHAPE, "H = 0 and C = 33": SHAPE, "C = 1 and id type 7": CLASSES,
        "N = 0 and id type 7": SHAPE, "C = 1 and h > H": CLASSES, "N = 0 and h > H": SHAPE, "bad flags and h > H": RANGE,
        "grad NULL and h > H": NULL,
    },
    "mas_teacher_loss_fwd": {
        "z NULL": NULL, "zt NULL": NULL, "spx NULL": NULL, "mask NULL": NULL, "bits NULL": NULL, "gmax NULL": NULL, "acc NULL": NULL,
        "flags: no fourth slot": RANGE, "flags: top1+ent": RANGE, "flags: within with ent": RANGE, "flags: rc": RANGE,
        "flags: tce": RANGE, "flags: wgroup": RANGE, "C = 1": CLASSES, "C = 33": CLASSES, "N = 0": SHAPE, "id type 7": DTYPE,
        "h > H": SHAPE, "w > W": SHAPE, "h > 0, w = 0": SHAPE, "invT_x = 0": RANGE, "invT_x NaN": RANGE, "z NULL and bad flags": NULL,
        "bad flags and N = 0": RANGE, "N = 0 and C = 1": SHAPE, "H = 0 and C = 33": SHAPE, "C = 1 and id type 7": CLASSES,
        "N = 0 and id type 7": SHAPE, "C = 1 and h > H": SHAPE, "N = 0 and h > H": SHAPE, "bad flags and h > H": RANGE,
        "acc NULL and h > H": SHAPE, "zt and z NULL": NULL, "zt NULL and bad flags": RANGE, "zt NULL and h > H": NULL,
    },
    "mas_teacher_loss_bwd": {
        "z NULL": NULL, "zt NULL": NULL, "spx NULL": NULL, "mask NULL": NULL, "bits NULL": NULL, "gmax NULL": NULL, "scale NULL": NULL,
        "fix NULL": NULL, "flags: no fourth slot": RANGE, "flags: top1+ent": RANGE, "flags: within with ent": RANGE, "flags: rc": RANGE,
        "flags: tce": RANGE, "flags: wgroup": RANGE, "C = 1": CLASSES, "C = 33": CLASSES, "N = 0": SHAPE, "id type 7": DTYPE,
        "h > H": SHAPE, "w > W": SHAPE, "h > 0, w = 0": SHAPE, "dz NULL at full resolution": NULL, "invT_x = 0": RANGE,
        "invT_x NaN": RANGE, "z NULL and bad flags": NULL, "bad flags and N = 0": RANGE, "N = 0 and C = 1": SHAPE,
        "H = 0 and C = 33": SHAPE, "C = 1 and id type 7": CLASSES, "N = 0 and id type 7": SHAPE, "C = 1 and h > H": SHAPE,
        "N = 0 and h > H": SHAPE, "bad flags and h > H": RANGE, "scale NULL and h > H": SHAPE, "zt and z NULL": NULL,
        "zt NULL and bad flags": RANGE, "zt NULL and h > H": NULL,
    },
    "mas_wgroup_loss_fwd": {
        "z NULL": NULL, "zt NULL": RANGE, "spx NULL": NULL, "mask NULL": NULL, "bits NULL": NULL, "gmax NULL": NULL, "tmax NULL": NULL,
        "acc NULL": NULL, "flags: no group": RANGE, "flags: no wgroup": RANGE, "flags: top1": RANGE, "flags: rc": RANGE,
        "flags: tce": RANGE, "C = 1": CLASSES, "C = 33": CLASSES, "N = 0": SHAPE, "id type 7": DTYPE, "h > H": SHAPE, "w > W": SHAPE,
        "h > 0, w = 0": SHAPE, "z NULL and bad flags": RANGE, "bad flags and N = 0": RANGE, "N = 0 and C = 1": SHAPE,
        "H = 0 and C = 33": SHAPE, "C = 1 and id type 7": CLASSES, "N = 0 and id type 7": SHAPE, "C = 1 and h > H": SHAPE,
        "N = 0 and h > H": SHAPE, "bad flags and h > H": RANGE, "acc NULL and h > H": SHAPE, "zt and z NULL": RANGE,
        "zt NULL and bad flags": RANGE, "zt NULL and h > H": RANGE,
    },
    "mas_wgroup_loss_bwd": {
        "z NULL": NULL, "zt NULL": RANGE, "spx NULL": NULL, "mask NULL": NULL, "bits NULL": NULL, "gmax NULL": NULL, "tmax NULL": NULL,
        "scale NULL": NULL, "fix NULL": NULL, "flags: no group": RANGE, "flags: no wgroup": RANGE, "flags: top1": RANGE,
        "flags: rc": RANGE, "flags: tce": RANGE, "C = 1": CLASSES, "C = 33": CLASSES, "N = 0": SHAPE, "id type 7": DTYPE, "h > H": SHAPE,
        "w > W": SHAPE, "h > 0, w = 0": SHAPE, "dz NULL at full resolution": NULL, "z NULL and bad flags": RANGE,
        "bad flags and N = 0": RANGE, "N = 0 and C = 1": SHAPE, "H = 0 and C = 33": SHAPE, "C = 1 and id type 7": CLASSES,
        "N = 0 and id type 7": SHAPE, "C = 1 and h > H": SHAPE, "N = 0 and h > H": SHAPE, "bad flags and h > H": RANGE,
        "scale NULL and h > H": SHAPE, "zt and z NULL": RANGE, "zt NULL and bad flags": RANGE, "zt NULL and h > H": RANGE,
    },
    "mas_loss_values": {
        "acc NULL": NULL, "losses NULL": NULL,
    },
    "mas_loss_scales": {
        "acc NULL": NULL, "grad NULL": NULL, "scale NULL": NULL,
    },
    "mas_loss_values_weighted": {
        "acc NULL": NULL, "weights NULL": NULL, "losses NULL": NULL,
    },
    "mas_loss_scales_weighted": {
        "acc NULL": NULL, "grad NULL": NULL, "weights NULL": NULL, "scale NULL": NULL,
    },
    "mas_teacher_loss_values": {
        "acc NULL": NULL, "losses NULL": NULL, "flags: no fourth slot": RANGE, "flags: top1+ent": RANGE, "flags: within with ent": RANGE,
        "flags: rc": RANGE, "flags: tce": RANGE, "flags: wgroup": RANGE,
    },
    "mas_teacher_loss_scales": {
        "acc NULL": NULL, "grad NULL": NULL, "scale NULL": NULL, "flags: no fourth slot": RANGE, "flags: top1+ent": RANGE,
        "flags: within with ent": RANGE, "flags: rc": RANGE, "flags: tce": RANGE, "flags: wgroup": RANGE,
    },
}


def answers(entry):
    lib, names, out = L.load(), ENTRIES[entry][0].split(), {}
    for label, override in _cases(entry).items():
        args = dict(_base(entry), **override)
        out[label] = getattr(lib, entry)(*[args[n] for n in names])
    return out


def test_the_table_names_every_scan_values_and_scales_entry_point():
    declared = [n for n in L.SIGNATURES if n.startswith(("mas_partial_loss_", "mas_teacher_loss_", "mas_wgroup_loss_", "mas_loss_"))
                and not n.endswith(("_reference", "_work_bytes"))]
    assert sorted(declared) == sorted(ENTRIES) == sorted(EXPECTED)
    for entry, (names, _, _) in ENTRIES.items():
        assert len(names.split()) == len(L.SIGNATURES[entry][1]), entry


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_refused_call_gets_the_code_it_always_got(entry):
    assert 0 not in EXPECTED[entry].values()
    assert answers(entry) == EXPECTED[entry]


def test_the_host_wrappers_refuse_target_rows_where_bit_masks_belong():
    """``bits`` goes to the library as a raw int32 [N,S] pointer: the u8 multi-hot rows [N,S,cols] it is formed from must not pass."""
    from mulactseg_amd import ops
    z = torch.zeros((N, C, H, W))
    spx, msk = torch.zeros((N, H, W), dtype=torch.int64), torch.ones((N, H, W), dtype=torch.uint8)
    rows = torch.ones((N, S, C), dtype=torch.uint8)
    for call in (lambda: ops.partial_loss_reference(z, spx, msk, rows, 1.0, CE),
                 lambda: ops.teacher_loss_reference(z, z, spx, msk, rows, 1.0, 1.0, 0.0, CE | TOP1),
                 lambda: ops.wgroup_loss_reference(z, z, spx, msk, rows, 1.0, CE | GROUP | WGROUP)):
        with pytest.raises(TypeError):
            call()
