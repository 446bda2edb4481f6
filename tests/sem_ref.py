"""Restatement of the mapper's semantic term (utils/mapper.py:863-866, 929-946, Decoder.sem_label_prob) for the tests
of `pings_amd.semantic_losses`: the reference's lines in torch, in whatever dtype the inputs have (the tests pass
float64).  Also Open3D's `remove_vertices_by_mask` (estimate_vertices_sem, utils/mesher.py:407-410) in numpy, for the
tests of `mesh_ops.remove_vertices`."""
import numpy as np
import torch


def nll(raw, w, y, freespace_on=False, d=1):
    """`raw` [B,k,S] with `w` [B,k] (or [B,k,1]), or [B,S] with `w` None (weighted_first); `y` integer labels [B]."""
    sem_pred = torch.nn.functional.log_softmax(raw, dim=-1)            # Decoder.sem_label_prob
    if w is not None:
        sem_pred = torch.sum(sem_pred * w.reshape(w.shape[0], w.shape[1], 1), dim=1)
    loss_nll = torch.nn.NLLLoss(reduction="mean")
    if freespace_on:
        label_mask = y >= 0
    else:
        label_mask = y > 0
    sem_pred = sem_pred[label_mask]
    sem_label = y[label_mask].long()
    return loss_nll(sem_pred[::d, :], sem_label[::d])


def selected_rows(y, freespace_on=False, d=1):
    """The rows the loss is taken over: `nonzero(label_mask)[::d]`."""
    return torch.nonzero(y >= 0 if freespace_on else y > 0).view(-1)[::d]


def remove_vertices_by_mask(verts, faces, drop):
    """Open3D's `TriangleMesh.remove_vertices_by_mask` in numpy: the vertices with `drop` go and every face naming one
    goes; kept vertices and kept faces keep their order and the faces are renumbered.
    -> (verts, faces, kept), `kept` the old index of every new vertex (per-vertex attributes follow as attr[kept])."""
    verts, faces, drop = np.asarray(verts), np.asarray(faces).reshape(-1, 3), np.asarray(drop, dtype=bool)
    keep = ~drop
    remap = np.where(keep, np.cumsum(keep) - 1, -1)
    fkeep = keep[faces].all(axis=1) if len(faces) else np.zeros(0, dtype=bool)
    return verts[keep], remap[faces[fkeep]].astype(faces.dtype).reshape(-1, 3), np.flatnonzero(keep)
