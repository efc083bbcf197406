#!/usr/bin/env python
"""Signatures of the compiled plans over a fixed matrix of (model, size, dtype policy, compiler switches, nosplit names, batch) -
no GPU needed.  One line per plan: SHA-256 of the serialised plan (Model.save_plan: everything the library is given) and of the
op names / kinds / MACs / fused ops (what the accounting reads; the serialised plan carries none of them), and the algorithmic
bytes per image; then how many ops of each fused block form the matrix produced.  A change to the compiler that claims to leave
the plans alone prints the same text before and after:
    python tools/plan_signature.py > after.txt"""
import collections
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yoloret_amd import compiler, layers as L, runtime as rt, weights as W   # noqa: E402
from yoloret_amd.yolo3.model import yolov3_body   # noqa: E402

MODELS = [('mobilenetv2x75', 416), ('mobilenetv2x14', 512), ('efficientnetb0', 416), ('efficientnetb0-lite', 416),
          ('efficientnetb3-lite', 320), ('mobilenetv2x75', 96), ('efficientnetb3', 224)]
POLICIES = ['float32', 'mixed_bfloat16']
BATCHES = [1, 8, 64]
SWITCHES = [{}, dict(MBR_SPLIT=False), dict(FUSE_MBR=False, FUSE_MBE=False), dict(FUSE_MBH=False), dict(FUSE_MBH=False, FUSE_MBX=False),
            dict(FUSE_STEMDW_MFMA=False), dict(STEM_MFMA=False), dict(FUSE_MBK=False), dict(MBN=False),
            dict(FUSE_MAX_CIN=1 << 20, FUSE_LANE_MIN_PIXELS=0, FUSE_MBR=False, FUSE_MBE=False, FUSE_MBK=False),
            dict(FUSE_STEM=False), dict(FUSE_STEMDW=False), dict(FUSE_LANE=False), dict(FUSE_LANE_NO_EXPAND=False),
            dict(MBR_BLOCKS=['block_7', 'block_8']), dict(MBH_SKIP={'32', '51'}), dict(FUSE_MBH=False, MBX_SKIP={'31', '52'})]
# (model, size, policy, nosplit names): plan ops taken off the split forms, as Model.check_ranges does - an mbr, an mbk and an mbe block
NOSPLIT = [('mobilenetv2x75', 416, 'float32', ['block_3_mbr', 'block_8_mbr', 'block_12_mbr'])]


def form(o):
    """The fused block form of plan op o (None: not an output of fuse_inverted_residuals)."""
    if o.kind == rt.OP_STEMBLOCK and o.name.endswith('_block0'):
        return 'stem+block0 ' + ('matrix-pipe' if 'scale' in o.params else 'float32-pipe')
    if o.kind == rt.OP_STEMBLOCK:
        return 'stem+depthwise ' + ('matrix-pipe entry' if o.k >> rt.STEMBLOCK_ENTRY_SHIFT else 'lane entry')
    if o.kind in (rt.OP_MBR, rt.OP_MBE):
        return ('mbr ' if o.kind == rt.OP_MBR else 'mbe ') + ('streaming' if o.k & rt.MBR_STREAM else 'split' if o.k & rt.MBR_SPLIT else 'plain')
    if o.kind == rt.OP_MBLANE:
        return 'mblane ' + ('with expand' if 'wgt' in o.params else 'without expand')
    return {rt.OP_MBH: 'mbh', rt.OP_MBX: 'mbx'}.get(o.kind)


def sha(b):
    return hashlib.sha256(b).hexdigest()


def main():
    forms = collections.Counter()
    cases = [(n, s, p, sw, ()) for n, s in MODELS for p in POLICIES for sw in SWITCHES] + [(n, s, p, {}, ns) for n, s, p, ns in NOSPLIT]
    for name, size, policy, sets, nosplit in cases:
        saved = {k: getattr(compiler, k) for k in sets}
        for k, v in sets.items():
            setattr(compiler, k, v)
        L.set_global_policy(policy)
        try:
            m = yolov3_body(L.Input(shape=[size, size, 3]), name, 3, num_classes=20)
            L.set_global_policy('float32')
            if nosplit:
                m._drop_split_forms(list(nosplit))
            m.set_weights(W.synthetic_weights(m, 1, 'conditioned'))
            for b in BATCHES:      # (the switches stay set: the plans of the smaller batches are compiled on first use)
                data, plan = m.save_plan(batch=b), m.plan_for(b)
                sig = repr([(o.name, o.kind, o.macs, [f.name for f in getattr(o, 'fused', ())]) for o in plan.ops])
                forms.update(f for f in map(form, plan.ops) if f)
                print('%s@%d %s %s nosplit=%s batch %d (%s): plan %s ops %s bytes/image %d' % (
                    name, size, policy, ','.join('%s=%s' % (k, sets[k] if not isinstance(sets[k], set) else sorted(sets[k])) for k in sorted(sets)) or '-',
                    ','.join(nosplit) or '-', b, m.variant(b), sha(data), sha(sig.encode()), plan.algorithmic_bytes_per_image()))
        finally:
            L.set_global_policy('float32')
            for k, v in saved.items():
                setattr(compiler, k, v)
    print('fused block forms over the matrix:')
    for f in sorted(forms):
        print('  %-34s %d' % (f, forms[f]))


if __name__ == '__main__':
    main()
