"""Seeded CPU inputs of the softmax-Dice suites (tests/test_dice_gpu.py, tests/test_labels_gpu.py) and the cases of the whole loss
family whose bits tests/golden/loss_family_bits.json records (tools/record_loss_bits.py writes the file, test_dice_gpu.py recomputes
every case)."""
import hashlib

import torch

BF, F32 = torch.bfloat16, torch.float32
CL = torch.channels_last_3d
SMALL, TRIPS = (5, 7, 9), (7, 11, 37)
DTYPES = {"f32": F32, "bf16": BF}


def logits_of(C, spatial, dtype, seed):
    return (3.0 * torch.randn(2, C, *spatial, generator=torch.Generator().manual_seed(seed))).to(dtype)


def labels_of(kind, C, spatial, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, C, (2,) + spatial, generator=g)
    if kind == "ignored":                      # values that are no class, 255 among them
        lab[torch.rand(lab.shape, generator=g) < 0.2] = C
        lab[torch.rand(lab.shape, generator=g) < 0.1] = 255
        lab[1, 0, 0, :2] = torch.tensor([C + 1 if C < 254 else 254, 255])
    elif kind == "absent":                     # class C - 1 never occurs in sample 0, class 0 never in sample 1
        lab[0][lab[0] == C - 1] = 0
        lab[1][lab[1] == 0] = C - 1
    elif kind == "single":                     # every voxel of sample 0 is class 1; sample 1 stays mixed
        lab[0] = 1
    return lab.to(torch.uint8)


def target_of(ct, spatial, seed, soft=False):
    """(2, ct, D, H, W) float32 target: a {0, 1} mask with 30 % foreground, or (soft) values uniform in [0, 1]."""
    r = torch.rand(2, ct, *spatial, generator=torch.Generator().manual_seed(seed))
    return r if soft else (r < 0.3).float()


# (C, ct, spatial) of the float form and (C, spatial) of the class-map forms (labels of kind "ignored"), each in both storage types.
# 5 * 7 * 9 = 315 voxels is odd: sample 1 starts misaligned and the 4-voxel path runs its head singles; TRIPS gives the forward
# about 3.7 trips.
FLOAT_BITS = [(2, 1, SMALL), (3, 3, SMALL), (5, 5, SMALL), (8, 8, SMALL), (2, 1, TRIPS), (3, 3, TRIPS)]
INDEX_BITS = [(C, SMALL) for C in (2, 3, 8, 9, 17, 32)] + [(C, TRIPS) for C in (2, 9)]
# ce and dice_ce: gamma = 2 with class weights at SMALL, gamma = 0 without at TRIPS; dice_ce: dice_weight 1, ce_weight 0.5
CE_BITS = INDEX_BITS
BOUNDARY_BITS = [(C, SMALL) for C in (2, 3, 8, 32)] + [(9, TRIPS)]
SLICE_BUFFER_C, SLICE_OFF, SLICE_C = 12, 4, 8      # boundary once more on channels [4, 12) of a 12-channel buffer: rows of 4, pitched


def _sp(spatial):
    return "x".join(str(s) for s in spatial)


def _boundary_ids(C):
    return (1,) if C == 2 else (0, C - 1)


def bit_cases():
    """[(case id, form, logits, target or labels, settings of the form)] on the CPU, in the order of the file."""
    out = []
    for name, dtype in DTYPES.items():
        for C, ct, sp in FLOAT_BITS:
            out.append(("float-C%d-ct%d-%s-%s" % (C, ct, _sp(sp), name), "float", logits_of(C, sp, dtype, 2100 + 10 * C + ct),
                        target_of(ct, sp, 2200 + 10 * C + ct), {}))
        for C, sp in INDEX_BITS:
            out.append(("index-C%d-%s-%s" % (C, _sp(sp), name), "index", logits_of(C, sp, dtype, 2300 + C), labels_of("ignored", C, sp, 2400 + C), {}))
        for form in ("ce", "dice_ce"):
            for C, sp in CE_BITS:
                kw = {"gamma": 2.0, "weight": 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(2700 + C))} if sp == SMALL else {"gamma": 0.0}
                out.append(("%s-C%d-%s-%s" % (form, C, _sp(sp), name), form, logits_of(C, sp, dtype, 2500 + C), labels_of("ignored", C, sp, 2600 + C), kw))
        for C, sp in BOUNDARY_BITS:
            out.append(("boundary-C%d-%s-%s" % (C, _sp(sp), name), "boundary", logits_of(C, sp, dtype, 2800 + C), labels_of("ignored", C, sp, 2900 + C),
                        {"ids": _boundary_ids(C)}))
        out.append(("boundary-C%d-of%d-%s-%s" % (SLICE_C, SLICE_BUFFER_C, _sp(SMALL), name), "boundary", logits_of(SLICE_BUFFER_C, SMALL, dtype, 3000),
                    labels_of("ignored", SLICE_C, SMALL, 3100), {"ids": _boundary_ids(SLICE_C), "channels": (SLICE_OFF, SLICE_C)}))
    return out


def device_bits(ops, form, z, t, gamma=0.0, weight=None, ids=None, channels=None):
    """One forward and backward on the device: the loss as its int32 bit pattern, and the sha256 of the gradient's bytes in NDHWC order."""
    x = z.cuda().contiguous(memory_format=CL)
    if channels is not None:                       # a channel slice of the wider buffer: the logits keep its voxel pitch
        x = x.narrow(1, *channels).detach()
    x.requires_grad_(True)
    t = t.cuda().contiguous(memory_format=CL) if form == "float" else t.cuda()
    if form == "float":
        loss = ops.softmax_dice_loss(x, t)
    elif form == "index":
        loss = ops.softmax_dice_index_loss(x, t)
    elif form == "ce":
        loss = ops.softmax_ce_index_loss(x, t, weight=None if weight is None else weight.cuda(), gamma=gamma)
    elif form == "dice_ce":
        loss = ops.softmax_dice_ce_index_loss(x, t, dice_weight=1.0, ce_weight=0.5, weight=None if weight is None else weight.cuda(), gamma=gamma)
    else:                                          # the map of the same labels: integer-exact on the device
        loss = ops.softmax_boundary_loss(x, ops.signed_sqdist(t, x.shape[1], ids), ids)
    loss.backward()
    raw = x.grad.permute(0, 2, 3, 4, 1).contiguous().cpu().view(torch.uint8).numpy().tobytes()
    return {"loss_bits": int(loss.detach().cpu().view(torch.int32)), "grad_sha256": hashlib.sha256(raw).hexdigest()}
