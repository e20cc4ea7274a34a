"""CPU self-tests of head_reference.py: the fp32 oracle in the kernel's place stays inside every cap on the chosen families, the hand-derived
labels of the dyadic scene are what the spec gives, float64 agrees with fp32 where the construction says so, and every K_REF is what it claims."""
import numpy as np
import torch

import head_reference as hr
from oracle import heads as oh

F = np.float32


def _within(worst, key):
    assert 0.5 * hr.K_REF[key] <= worst <= hr.K_REF[key], (key, worst, hr.K_REF[key])


def test_dyadic_assignment_families_fp32_float64_and_hand_derived_labels():
    cases = hr.assign_cases()
    assert {len(c.anchors) for c in cases} >= {1, 255, 257, 131072 + 257}
    assert {c.gt.shape[1] for c in cases if not c.coded} >= {0, 1, 127, 128} and {c.gt.shape[1] for c in cases if c.coded} >= {255, 256}
    assert {c.gt.shape[0] for c in cases} >= {1, 3}
    fails = []
    for c in cases:
        s = c.spec
        f, _ = c.check(s["labels"], s["t32"], s["weights"], hr.K_REF["encode"])   # also: the spec against the hand-derived expectations
        fails += f
        lab64, arg64, _ = c.spec64
        skip = hr.dyadic_f64_exceptions(c) if c.expect else np.zeros_like(lab64, bool)
        if ((lab64 != s["labels"]) & ~skip).any() or ((arg64 != s["arg"]) & ~skip).any():
            fails.append("%s: float64 and fp32 decide differently off the listed exceptions" % c.name)
        if not c.coded and c.per_loc > 1 and c.E == 0 and len(c.anchors) % c.per_loc == 0:       # the layout oracle.heads.assign_targets takes
            lo, to, wo = oh.assign_targets(c.anchors, np.diff(c.offs).tolist(), c.set_class.tolist(), c.mthr, c.uthr, c.gt)
            if not (np.array_equal(lo, s["labels"]) and np.array_equal(to.view(np.int32), s["t32"].view(np.int32)) and np.array_equal(wo, s["weights"])):
                fails.append("%s: the restated spec and oracle.heads.assign_targets differ" % c.name)
    assert not fails, "\n".join(fails)
    scene = cases[0]
    assert len(scene.expect) >= 60 and {v[0] for v in scene.expect.values()} >= {-1, 0, 1, 2, 3, 4, 5, 6}
    # fp32 rules where float64 disagrees: IoU 3/5 against matched 0.6 is positive in fp32 (3/5 rounds to float32(0.6)) and not in float64
    lab64 = scene.spec64[0]
    dis = np.argwhere(lab64 != scene.spec["labels"])
    assert len(dis) == 1 and scene.spec["labels"][tuple(dis[0])] == 4 and lab64[tuple(dis[0])] == -1


def test_random_assignment_family_margin_cap_and_encode_k_ref():
    c = hr.random_assign_case()
    s = c.spec
    decided = hr.decided_by_margin(c)
    assert (~decided).mean() <= hr.UNDECIDED_CAP, (~decided).mean()
    assert np.array_equal(c.spec64[0][decided], s["labels"][decided])           # the fp32 oracle in the kernel's place
    assert (s["labels"] > 0).sum() >= 50 and (s["labels"] < 0).sum() >= 10 and (s["labels"] == 0).sum() >= 1000
    worst = 0.0
    for case in [c] + hr.assign_cases():
        fails, w = case.check(case.spec["labels"], case.spec["t32"], case.spec["weights"], hr.K_REF["encode"])
        assert not fails, fails
        worst = max(worst, w)
    _within(worst, "encode")


def test_decode_families_spec_equals_oracle_and_k_ref():
    worst = 0.0
    cases = hr.decode_cases() + [hr.stride_decode_case()]
    assert {c.num_bins for c in cases if c.dir_logits is not None} == {1, 2, 3, 4, 9}
    for c in cases:
        fails, w = c.check(c.spec["boxes"], hr.K_REF["decode"])
        assert not fails, fails
        worst = max(worst, w)
        if c.dir_logits is not None and not c.coded:
            o = oh.generate_predicted_boxes(c.enc, c.anchors, c.dir_logits, c.dir_offset, c.dir_limit_offset, c.num_bins)
            assert np.array_equal(o.view(np.int32), c.spec["boxes"].view(np.int32)), c.name
    _within(worst, "decode")
    # the boundary family does sit on the floor's edge: neighbouring headings get different period counts, and the period built in fp32
    # (2.0f * pi / 9) is an ulp off float32(2 pi / 9) and moves some of them; for 1 .. 8 bins the two periods are one number
    for nb in (1, 2, 3, 4, 9):
        c = hr.boundary_decode_case(nb, 0.0)
        k = c.spec["k"][0]
        assert (np.diff(k.reshape(-1, 7), axis=1) != 0).any(1).sum() >= 7
        per32 = F(2.0) * F(np.pi) / F(nb)
        moved = int((np.floor((c.enc[0, :, 6] - F(c.dir_offset)) / per32 + F(0.0)) != k).sum())
        assert (per32 != F(2 * np.pi / nb)) == (nb == 9) and (moved > 0) == (nb == 9), (nb, moved)


def test_radius_family_chain_torch_and_oracle():
    h, w, mo = hr.radius_family()
    assert len(h) >= 200
    spec = hr.radius_spec_family()
    ints = spec.astype(int)
    assert set(range(2, 13)) <= set(ints.tolist())
    assert (ints.reshape(-1, 7).min(1) != ints.reshape(-1, 7).max(1)).sum() >= 30          # the +-3 ulp neighbours straddle the integer
    # the reference's own lines on torch-CPU tensors, Python scalars entering as torch takes them: the same bits once the square root is the
    # correctly rounded one (torch's vectorised CPU sqrt is faithfully, not correctly, rounded: it is off in the last bit on about 0.6 % of random
    # arguments, which is all of the bit differences between the numpy oracle and the raw torch chain on random sizes)
    tx = np.concatenate([hr.radius_chain_torch(h[mo == m], w[mo == m], m, exact_sqrt=True) for m in (0.1, 0.5, 0.7)])
    assert np.array_equal(tx.view(np.int32), spec.view(np.int32))
    raw = np.concatenate([hr.radius_chain_torch(h[mo == m], w[mo == m], m) for m in (0.1, 0.5, 0.7)])
    orc = np.array([F(oh.gaussian_radius(F(a), F(b), F(m))) for a, b, m in zip(h, w, mo)])
    print("radius family: %d sizes; integer part differs from the spec: raw torch chain %d, oracle.heads.gaussian_radius %d" %
          (len(h), int((raw.astype(int) != ints).sum()), int((orc.astype(int) != ints).sum())))
    assert np.array_equal(orc.astype(int), ints)
    rng = np.random.default_rng(0)
    x = rng.uniform(0.1, 2000, 20000).astype(F)
    assert np.array_equal(np.sqrt(x), np.sqrt(x.astype(np.float64)).astype(F))               # numpy's is the correctly rounded one


def test_center_families_k_ref_and_transposition():
    worst = 0.0
    cases = hr.center_cases()
    assert {c.gt.shape[1] for c in cases} >= {0, 63, 64, 65, 255, 256, 257, 600} and {c.num_max_objs for c in cases} == {5, 500}
    for c in cases:
        for cc in (c, c.swapped()):
            assert cc.W != cc.H and cc.voxel[0] != cc.voxel[1]
            got = {k: [np.asarray(a) for a in v] for k, v in cc.spec.items()}
            fails, w, ulp = cc.check(got, hr.K_REF["center_boxes"])
            assert not fails and ulp == 0, fails
            worst = max(worst, w)
        if c.name.startswith("radius family"):
            continue                                                            # (c w) h is not (c h) w in the last bit: an ulp decides the radius there
        a, b = c.spec, c.swapped().spec                                          # elsewhere the swapped call is the transposed problem
        for h in range(len(c.each_head)):
            assert np.array_equal(a["masks"][h], b["masks"][h])
            ia, ib = a["inds"][h], b["inds"][h]
            assert np.array_equal((ia % c.W) * c.H + ia // c.W, ib)
            assert np.array_equal(a["heatmaps"][h].transpose(0, 1, 3, 2), b["heatmaps"][h])
    _within(worst, "center_boxes")
    # the family has what it says: clamped centres, a skipped box with later slots in rank, truncation inside a chunk
    c = [c for c in cases if c.name == "centres and windows"][0]
    assert c.spec["masks"][0][0].sum() == 24 and c.spec["masks"][0][0][24] == 0 and c.spec["masks"][0][0][25] == 0
    r = [c for c in cases if c.name.startswith("ranking G=600") and c.num_max_objs == 500][0]
    holes = [int(np.nonzero(m[0])[0].max() + 1 - m[0].sum()) for m in r.spec["masks"]]
    assert sorted(holes) == [0, 0, 1], holes                                     # the dx = 0 box keeps its slot masked off, later boxes keep their rank


def test_loss_families_k_ref():
    worst = dict(focal=0.0, focal_grad=0.0, smooth_l1=0.0, smooth_l1_grad=0.0)
    for c in hr.focal_cases() + hr.smooth_l1_cases() + [hr.stride_loss_inputs("focal"), hr.stride_loss_inputs("smooth_l1")]:
        v, g = c.chain32()
        assert torch.isfinite(v).all()
        rv, rg = c.ratios(v.numpy(), g.numpy())
        worst[c.kind] = max(worst[c.kind], rv)
        worst[c.kind + "_grad"] = max(worst[c.kind + "_grad"], rg)
        assert c.documented_zero(g.numpy())
    for k, w in worst.items():
        _within(w, k)
    assert sum(int(c.ref[4].sum()) for c in hr.focal_cases()) > 0                # float64 does meet its infinite gradient (gamma < 1 at pt = 0)
    # |d| = beta is hit exactly.  At 1/9, 1 and 1e-5 both branches of the smooth-L1 give 0.5 beta there bit for bit, so the comparison does not
    # show; at BETA_BRANCHES_DIFFER they differ, the reference's chain takes the linear one (`n < beta` is false), and the GPU test holds the
    # kernel's value to the chain's bits: `<` against `<=` is pinned there
    seen = set()
    for c in hr.smooth_l1_cases():
        if "(+0 ulp)" in c.name and c.kw["beta"] >= 1e-5:
            b = F(c.kw["beta"])
            cw = np.ones(c.x.shape[-1], F) if c.kw.get("cw") is None else c.kw["cw"].numpy()
            d = (c.x - torch.where(torch.isnan(c.t), c.x, c.t)).numpy() * cw
            on = np.abs(d) == b
            assert on.sum() >= 1, c.name
            differ = bool(F(0.5) * (b * b) / b != b - F(0.5) * b)
            assert differ == (c.kw["beta"] == hr.BETA_BRANCHES_DIFFER)
            if differ and (c.w is None or bool((c.w != 0).any())):
                v = c.chain32()[0].numpy()
                wt = np.ones(c.x.shape[:2], F) if c.w is None else c.w.numpy()
                lin, quad = (b - F(0.5) * b) * wt[..., None], (F(0.5) * (b * b) / b) * wt[..., None]
                assert np.array_equal(v[on], np.broadcast_to(lin, v.shape)[on]) and (np.broadcast_to(quad, v.shape)[on] != v[on]).any()
                seen.add(c.w is None)
    assert seen == {True, False}


def test_radius_family_heat_map_shows_every_members_radius():
    """Each member of the radius family has a heat-map channel of its own, and an integer radius one too small or one too large changes that
    channel, in the call as it stands and with x and y exchanged: a kernel that gets any member's radius wrong cannot pass."""
    cases = [c for c in hr.center_cases() if c.name.startswith("radius family")]
    assert len(cases) == 3 and sum(c.gt.shape[1] for c in cases) >= 200
    for c in cases:
        for cc in (c, c.swapped()):
            n = cc.gt.shape[1]
            ref = cc.spec["heatmaps"][0]
            assert ref.shape[:2] == (1, n) and int(cc.spec["masks"][0].sum()) == n
            for delta in (-1, 1):
                moved = cc.spec_heat(delta)[0]
                same = [i for i in range(n) if np.array_equal(moved[0, i], ref[0, i])]
                assert not same, (cc.name, delta, same)
