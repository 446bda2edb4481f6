"""Golden vectors of the loop-closure context from the reference's own functions and manager (utils/loop_detector.py).

Runs `ptcloud2sc_torch`, `sc2rk`, `distance_sc_torch`, `distance_sc_feature_torch` and a `NeuralPointMapContextManager`
sequence (add_node x K, set_virtual_node, detect_loop) on the CPU through `oracle.ref_shim.load()` and writes
tests/golden/loop_context.npz, loop_distance.npz and loop_sequence.npz: inputs, config scalars and outputs.  Feature
values are stored as float16 (they are exact in float32).  tests/test_loop_ops.py reads only the files.

    python tools/make_loop_golden.py            (needs the reference tree; CPU only)
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import loop_ref as LR  # noqa: E402
from oracle import ref_shim  # noqa: E402

K_NODES, FRAME_STEP = 12, 7          # frame ids 0, 7, ..., 77: the bank of loop_ops grows once on the way


def reference():
    R = ref_shim.load()
    import utils.loop_detector as ld  # type: ignore

    return R, ld


def f16(t):
    return t.half().float()


def context_fixture(ld):
    fp = LR.pose()
    pts = LR.to_sensor(LR.field(1200, seed=3), fp)
    feats = f16(LR.features(pts, 8, seed=3))
    out = dict(points=pts.numpy(), features=feats.numpy().astype(np.float16), max_length=np.float64(60.0))
    for tag, shape in (("a", [20, 60]), ("b", [3, 7])):
        sc, scf = ld.ptcloud2sc_torch(pts, feats, shape, 60.0)
        sc0, none = ld.ptcloud2sc_torch(pts, None, shape, 60.0)
        assert none is None and torch.equal(sc, sc0)
        out.update({f"shape_{tag}": np.array(shape), f"sc_{tag}": sc.numpy(), f"scf_{tag}": scf.numpy(),
                    f"rk_{tag}": ld.sc2rk(sc).numpy(), f"rkf_{tag}": ld.sc2rk(scf).numpy()})
    return out


def distance_fixture(ld):
    out = {}
    for i, (feature, tie) in enumerate(((False, None), (False, "period"), (True, None))):
        c = LR.search_case(3, 3, feature, seed=11 + i, tie=tie)
        a, b = c["ctx"][c["cand"][c["cw"]]], c["q_ctx"][c["qw"]]
        if feature:
            a, b = f16(a), f16(b)
        d, yaw = (ld.distance_sc_feature_torch if feature else ld.distance_sc_torch)(a, b)
        store = (lambda t: t.numpy().astype(np.float16)) if feature else (lambda t: t.numpy())
        out.update({f"a_{i}": store(a), f"b_{i}": store(b), f"dist_{i}": np.float64(d), f"yaw_{i}": np.int64(yaw)})
    out["count"] = np.int64(3)
    return out


def sequence_poses():
    """K poses on a circle of radius 25 m through the field's centre, heading along the tangent.  The last one is placed
    so that its virtual pose 4 m to the side (index side_count + 2) stands 0.4 m from where node 0 stood, turned by four
    sectors (24 degrees); the one before it fixes the direction of travel the reference derives the side from."""
    c = np.array([150.0, -80.0, 3.0])
    poses = []
    for k in range(K_NODES - 2):
        phi = 2 * np.pi * k / (K_NODES - 1)
        pos = c + 25.0 * np.array([np.cos(phi) - 1.0, np.sin(phi), 0.0])
        poses.append(LR.pose(tuple(pos), phi + np.pi / 2))
    yaw = np.pi / 2 + np.radians(24.0)
    a = 1.0                                              # direction of travel (world), as the reference reads it
    d, v = np.array([np.cos(a), np.sin(a), 0.0]), np.array([-np.sin(a), np.cos(a), 0.0])
    rot = LR.pose((0.0, 0.0, 0.0), yaw)[:3, :3].numpy()
    last = c - rot @ (4.0 * v) + np.array([0.35, -0.2, 0.0])     # not exactly: the descriptors differ a little
    poses.append(LR.pose(tuple(last - 2.5 * d), yaw))
    poses.append(LR.pose(tuple(last), yaw))
    return torch.stack(poses)


def smooth_features(points, d):
    """Features that vary slowly over the field (a descriptor of them means something), exact in float16."""
    p = points.double()
    cols = [torch.sin(p[:, 0] * (0.03 + 0.011 * i) + p[:, 1] * (0.05 - 0.007 * i) + 0.9 * i) for i in range(d)]
    return f16(torch.stack(cols, dim=1).float())


def sequence_fixture(ld, R):
    poses = sequence_poses()
    pts = LR.field(1900, seed=5)
    # leave only points every pose of the sequence can decide in fp32 (tests/loop_ref.py: decidability)
    drop = torch.zeros(pts.shape[0], dtype=torch.bool)
    for k in range(K_NODES):
        drop |= LR.undecidable_points(LR.to_sensor(pts, poses[k]), LR.IDENTITY, 20, 60, 60.0)
    T, _, _ = LR.virtual_transforms(poses[-1], poses[-2], 5, 2.0)
    drop |= LR.undecidable_points(pts, T, 20, 60, 60.0)
    pts = pts[~drop].contiguous()
    feats = smooth_features(pts, 8)
    frame_ids = np.arange(K_NODES) * FRAME_STEP
    fix = dict(points=pts.numpy(), features=feats.numpy().astype(np.float16), poses=poses.numpy(),
               frame_ids=frame_ids, candidates=frame_ids[[4, 0, 2, 1, 3]].copy(), end_frame=np.int64(100),
               cosdist_threshold=np.float64(0.2))
    for tag, use_feature in (("plain", False), ("feature", True)):
        cfg = R.make_config(end_frame=100, loop_with_feature=use_feature, local_map_context=True,
                            context_cosdist_threshold=0.2)
        ref_module = type("M", (), {"NeuralPointMapContextManager": lambda cfg_, _c=cfg: ld.NeuralPointMapContextManager(_c)})
        mgr, triple = LR.run_sequence(ref_module, fix, use_feature)
        assert triple[0] is not None, f"the {tag} sequence must close a loop: {triple}"
        fix[f"loop_id_{tag}"] = np.int64(triple[0])
        fix[f"cosdist_{tag}"] = np.float64(triple[1])
        fix[f"T_{tag}"] = np.asarray(triple[2], dtype=np.float64)
        fix[f"ringkeys_{tag}"] = torch.stack([(mgr.ringkeys_feature if use_feature else mgr.ringkeys)[i]
                                              for i in frame_ids]).numpy()
        if not use_feature:
            fix["context0_plain"] = mgr.contexts[0].numpy()
        fix[f"query_ringkeys_{tag}"] = torch.stack([ld.sc2rk(q) for q in mgr.query_contexts]).numpy()
        fix[f"tran_from_frame_{tag}"] = torch.stack(mgr.tran_from_frame).numpy()
        print(tag, "loop", triple[0], "cosdist", triple[1])
    return fix


def main():
    R, ld = reference()
    out_dir = ROOT / "tests" / "golden"
    for name, fix in (("loop_context", context_fixture(ld)), ("loop_distance", distance_fixture(ld)),
                      ("loop_sequence", sequence_fixture(ld, R))):
        path = out_dir / f"{name}.npz"
        np.savez_compressed(path, **fix)
        print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
