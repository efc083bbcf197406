"""Pins tests/depthwise_geo.py - the Python restatement of the depthwise launch geometry - and the case tables built from it: what
tests/test_gpu_depthwise_forms.py relies on to reach every tile class, every walk and every instantiation.  No GPU."""
import os
import re

from tests import depthwise_geo as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    return open(os.path.join(ROOT, 'yoloret_amd', 'csrc', name)).read()


def test_mirror_agrees_with_the_compiler():
    """For every map 1..80 x 1..80: the tiles along x / y of the LDS-tiled form (3 x 3 and 5 x 5, plain and squeeze-excite), the rows of
    the walking form's sums and the squeeze-excite geometry of dw_kernel equal the compiler's, which sizes the plans' buffers with them
    (a launcher refuses a buffer of another height: tests/test_gpu_narrow.py)."""
    from yoloret_amd import compiler
    for h in range(1, G.SWEEP + 1):
        for w in range(1, G.SWEEP + 1):
            for k in (3, 5):
                for se in (False, True):
                    g = G.dwp_geometry(h, w, k, se)
                    assert (g.ntx, g.nty) == compiler.dwp_geometry(h, w, k, se), (h, w, k, se)
                    assert 1 <= g.nbig <= g.nband and g.nbig * g.R + (g.nband - g.nbig) * (g.R - 1) == g.th, (h, w, k, se, g)
                    assert g.ntx * g.tw >= w > (g.ntx - 1) * g.tw and g.nty * g.th >= h > (g.nty - 1) * g.th
            if compiler.DW_WALK:
                for b in (1, 2, 3):
                    for se in (False, True):
                        q = G.dwq_geometry(h, w, b, 5, se)
                        assert (q.nblk, q.nq) == compiler.dwl_geometry(h, w, 5), (h, w, b, se)
                        assert q.Q % 5 == 0 and (q.nq - 1) * q.Q < h <= q.nq * q.Q
                        assert q.nblk * q.spb * 4 >= w and q.ni * q.spb <= 8 and q.nw == (q.ni * q.spb + 1) // 2 <= 4
    for strips in (1, 2, 7, 85, 86, 300, 4290):
        for c4 in list(range(1, 300)) + [1024]:
            assert G.dw_se_geometry(strips, c4) == compiler.dw_se_geometry(strips, c4)


def test_mirror_constants_are_the_sources():
    """The numbers the mirror restates, read from the .hip files: a change there must come with a change here."""
    lds, walk, dw = _src('depthwise_lds.hip'), _src('depthwise_walk.hip'), _src('depthwise.hip')
    assert 'constexpr int DWP_MAX_R = %d;' % G.DWP_MAX_R in lds
    assert 'const int cap = se ? 192 : 208;' in lds
    assert 'const int row_cost = K * K * 4 + 21, in_cost = 3 * (4 + halo), round_cost = 12, tile_cost = 60;' in lds
    assert 'for (int tw = 8; tw <= 32; tw += 8)' in lds
    assert ': 3 * 256;' in lds and G.DWP_SLOTS == 768
    assert [int(r) for r in re.findall(r'case (\d): (?:if constexpr \(K == 3\) )?return launch_dwp_r<T, K, SE, \1>', lds)] == [1, 2, 3, 4, 5, 6]
    assert 'const int wave_cap = K == 5 ? 12 : 16;' in walk and 'int pc = (int)(160 * 1024 / l);' in walk
    assert 'if ((K * ni * a->U + nw - 1) / nw > 10) continue;' in walk
    assert 'const bool big = lanes >= (1ll << 21);' in dw and G.DW_BIG_LANES == 1 << 21
    assert 'return dw_pick_plain<T>(op.k, op.stride, (long long)batch * a.Ho * a.Wo * a.C4)(a, s);' in dw          # what `lanes` is
    # the instantiations of the plain form outside YR_DW_EXPERIMENT builds: the rest of dw_pick_plain, which holds the `big` rule
    tail = dw[dw.index('const bool big ='):]
    tail = tail[:tail.index('\n}\n')]
    assert tail.count('return ') == 4
    assert sorted(set(tuple(int(v) for v in m) for m in re.findall(r'launch_dw<(\d), (\d), (\d), (\d), T>', tail))) == sorted(G.DW_INSTANCES)


def test_dwp_case_tables_reach_every_class():
    """37 classes (tw, th, R, nband, nbig) of the plain 3 x 3 form, 33 of the squeeze-excite form; every R the launcher can pick and
    every tile width; each class has a single-tile witness, and a ragged map of 2 x 2 tiles or more wherever the class has one at all
    (a class whose tile is lower than its width's cap exists only on maps of one tile row)."""
    for se, n, rs in ((False, 37, {1, 2, 3, 4, 5, 6}), (True, 33, {1, 2, 3, 4, 5})):
        cases = G.dwp_class_cases(se)
        swept = {G.dwp_class(G.dwp_geometry(h, w, 3, se)) for h in range(1, G.SWEEP + 1) for w in range(1, G.SWEEP + 1)}
        assert len(cases) == n and {c for c, _, _ in cases} == swept
        assert {c[2] for c in swept} == rs and {c[0] for c in swept} == {8, 16, 24, 32}
        wider = set()        # classes with a ragged map of 2 x 2 tiles or more among maps up to twice the sweep
        for h in range(1, 2 * G.SWEEP + 1):
            for w in range(1, 2 * G.SWEEP + 1):
                g = G.dwp_geometry(h, w, 3, se)
                if g.ntx >= 2 and g.nty >= 2 and h % g.th and w % g.tw:
                    wider.add(G.dwp_class(g))
        ragged = 0
        for cls, one, many in cases:
            g = G.dwp_geometry(one[0], one[1], 3, se)
            assert G.dwp_class(g) == cls and (g.ntx, g.nty) == (1, 1)
            assert any(one[0] <= a and one[1] <= b for a, b in ((18, 1), (9, 9), (6, 17), (4, 25))), one
            if many is None:
                assert cls not in wider, cls
                continue
            ragged += 1
            g = G.dwp_geometry(many[0], many[1], 3, se)
            assert G.dwp_class(g) == cls and g.ntx >= 2 and g.nty >= 2 and many[0] % g.th and many[1] % g.tw
        assert ragged >= 12


def test_dwp_walk_cases_have_the_runs():
    """The multi-tile cases: run lengths 1, 2 and 3 (both buffer parities at the end of a run), a run that passes into the next tile
    row and one that passes into the next image - in the plain and in the squeeze-excite form."""
    for se in (False, True):
        lengths, row_cross, image_cross = set(), False, False
        for h, w, b in G.WALK_CASES:
            g = G.dwp_geometry(h, w, 3, se)
            ln, rc, ic = G.dwp_run_facts(b, G.WALK_C, g)
            runs = G.dwp_runs(b, G.WALK_C, g)
            assert len(runs) == 48 and runs[0][0] == 0 and runs[-1][1] == b * g.ntx * g.nty
            assert all(a[1] == c[0] for a, c in zip(runs, runs[1:]))
            lengths |= ln
            row_cross |= rc
            image_cross |= ic
        assert {1, 2, 3} <= lengths and row_cross and image_cross, (se, lengths, row_cross, image_cross)
    # the largest op-level case before these (52 x 52 x 128, batch 2): one tile per walker
    assert G.dwp_run_facts(2, 128, G.dwp_geometry(52, 52, 3, False))[0] == {1}


def test_dwq_case_table_reaches_every_class():
    """All (spb, ni, nw, U) classes of square maps 1..80 at batch 1 and 2 - ten in the plain form, ten in the squeeze-excite form (its
    sums take LDS, which moves the two-image choice) -; last quanta of 1, 2, 3 and 4 rows; maps lower than the kernel; odd batches
    in the two-image classes; more than one column block."""
    for se in (False, True):
        swept = {G.dwq_class(G.dwq_geometry(n, n, b, 5, se)) for n in range(1, G.SWEEP + 1) for b in (1, 2)}
        assert len(swept) == 10
        if not se:
            assert swept == {(1, 1, 1, 1), (2, 1, 1, 2), (2, 2, 2, 2), (3, 1, 2, 2), (3, 2, 3, 2), (4, 1, 2, 3), (5, 1, 3, 3), (6, 1, 3, 4),
                             (7, 1, 4, 4), (8, 1, 4, 5)}
        geos = [(h, w, b, G.dwq_geometry(h, w, b, 5, se)) for h, w, b in G.DWQ_CASES]
        assert {G.dwq_class(g) for _, _, _, g in geos} == swept
        assert {1, 2, 3, 4} <= {G.dwq_last_quantum(h, g) for h, _, _, g in geos if g.nq > 1}
        assert {g.ni for _, _, b, g in geos if b % 2} >= {1, 2}
        two = {G.dwq_class(g) for _, _, b, g in geos if g.ni == 2 and b % 2}
        assert two == {c for c in swept if c[1] == 2}
        assert any(h == 1 for h, _, _, _ in geos) and any(1 < h < 5 for h, _, _, _ in geos) and any(g.nblk > 1 for _, _, _, g in geos)


def test_dwq_segment_cases_walk_several_quanta():
    """The class cases all run one quantum per segment (so do the 64-channel batches of 301 and 400 of tests/test_gpu_narrow.py); the
    segment cases run a whole image of three quanta and two segments of two quanta, each ending in a short quantum."""
    for se in (False, True):
        assert all(G.dwq_segments(h, w, b, c, 5, se)[0] == 1 for h, w, b in G.DWQ_CASES for c in (G.DWP_C, G.TAIL_C))
        assert G.DWP_C % 8 == 0 and G.TAIL_C % 8 and G.DWP_C // 64 == G.TAIL_C // 64 == 1      # a chunk and a tail; a vector cut short
        assert [G.dwq_segments(h, w, b, 64, 5, se) for h, w, b in ((26, 26, 400), (33, 20, 301))] == [(1, 2), (1, 3)]
        got = [(G.dwq_segments(h, w, b, G.WALK_C, 5, se), G.dwq_geometry(h, w, b, 5, se).nq) for h, w, b in G.DWQ_SEG_CASES]
        assert got == [((3, 1), 3), ((2, 2), 4)], got
    walk = _src('depthwise_walk.hip')
    assert 'const int row_cost = K * K * 5 + 45, in_cost = 30, seg_cost = 600;' in walk
    assert 'const long long slots = 256ll * per_cu, units = (long long)a->ncc * a->nig * a->nblk;' in walk
    assert 'if (best == 0 || cost <= best) {' in walk


def test_dw_kernel_cases_reach_every_instantiation():
    seen = set()
    for dt, vec in (('f32', 4), ('bf16', 8), ('f16', 8)):
        c = G.DW_SMALL_C[dt]
        assert c < 64 and c % vec
        for k, s, h, w, b in G.DW_SMALL_CASES:
            seen.add(G.dw_instance(k, s, b, h, w, c, vec))
            assert b * -(-h // s) * -(-w // s) * -(-c // vec) > 256          # more than one workgroup
        big, below = G.dw_big_batches()
        h, w = G.DW_BIG_HW
        cb = G.DW_BIG_C[dt]
        assert cb % vec and h % 2 and w % 2 and ((h + 1) // 2) % 2        # a channel tail; odd Ho: the last row pair is half empty
        assert G.dw_instance(3, 2, big, h, w, cb, vec) == (3, 2, 2, 2) and G.dw_instance(3, 2, below, h, w, cb, vec) == (3, 2, 2, 1)
        assert below == big - 1 and big % G.DW_BIG_DISTINCT
        seen.add((3, 2, 2, 2))
    assert seen == set(G.DW_INSTANCES) and len(seen) == 5
    # the squeeze-excite form: cw = C4 dividing 256, cw = C4 not dividing 256, 32-vector blocks with several workgroups per strip group
    kinds = set()
    for dt, k, s, h, w, c, b in G.DW_SE_CASES:
        vec = 4 if dt == 'f32' else 8
        assert dt == 'f32' or s == 2 or c < 64          # else the 16-bit map goes to the LDS-tiled forms
        c4 = -(-c // vec)
        cw, ncb, rows = G.dw_se_geometry(-(-h // s) * -(-(-(-w // s)) // (4 if s == 1 else 2)), c4)
        kinds.add('cw=c4|256' if cw == c4 and 256 % cw == 0 else 'cw=c4' if cw == c4 else 'blocks>1' if ncb > 1 else 'blocks')
        if ncb > 1:
            assert c4 % 32           # the last block is cut short
    assert kinds >= {'cw=c4|256', 'cw=c4', 'blocks>1'}
    assert {(k, s) for _, k, s, _, _, _, _ in G.DW_SE_CASES} == {(3, 1), (3, 2), (5, 1), (5, 2)}


def test_no_case_exceeds_the_size_cap():
    """No tensor beyond 20 MB - but the big-branch case of dw_kernel, below 150 MB."""
    worst = 0
    for se in (False, True):
        for _, one, many in G.dwp_class_cases(se):
            for hw in (one, many):
                if hw:
                    worst = max(worst, 2 * hw[0] * hw[1] * (G.round_up(G.TAIL_C, 8) + 16) * 2)
    for h, w, b in G.WALK_CASES + G.DWQ_SEG_CASES:
        worst = max(worst, b * h * w * (G.WALK_C + 16) * 2, b * h * G.WALK_C * 4)       # (a row two vectors wider; the sums: fewer rows than h)
    for h, w, b in G.DWQ_CASES:
        worst = max(worst, b * h * w * (G.round_up(G.TAIL_C, 8) + 16) * 2)
    for k, s, h, w, b in G.DW_SMALL_CASES:
        worst = max(worst, b * h * w * 64 * 4)
    for dt, k, s, h, w, c, b in G.DW_SE_CASES:
        worst = max(worst, b * h * w * (c + 16) * 4)
    assert worst <= G.MAX_BYTES, worst
    big, _ = G.dw_big_batches()
    for dt, es, vec in (('f32', 4, 4), ('bf16', 2, 8), ('f16', 2, 8)):
        ld = G.round_up(G.DW_BIG_C[dt], vec)
        assert G.MAX_BYTES < big * G.DW_BIG_HW[0] * G.DW_BIG_HW[1] * ld * es <= G.MAX_BYTES_BIG
