"""Image pairs from global descriptors on the HIP backend.

Drop-in for imcui/hloc/pairs_from_retrieval.py: `main`, `parse_names`, `get_descriptors` and `pairs_from_score_matrix` with the
reference's signatures and the same output file (one `query db` line per pair, no trailing newline).  The feature files are read through
`utils.h5lite` (h5py when installed).  The similarity matrix (:109), the `invalid` mask, `min_score` and the top-k (:56-66) run on the
device in ONE library entry (imcui_hip_retrieval_topk): the score matrix is never read back, only the [Q, num_select] indices and scores.

Intended divergence: equal scores go to the LOWER database index (`torch.topk` leaves that order open), and `num_select` above the number
of database images is served (the missing ranks are skipped) where `torch.topk` raises.  `db_model` (a COLMAP `images.bin`) is refused.
"""
from __future__ import annotations

import argparse
import collections.abc as collections
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from .. import backend
from .extract_features import list_h5_names
from .utils.h5lite import open_h5


def parse_image_list(path):
    """imcui/hloc/utils/parsers.py:11-31 without intrinsics: the first word of every line that is neither empty nor a comment."""
    images = []
    with open(path, "r") as f:
        for line in f:
            line = line.strip("\n")
            if len(line) == 0 or line[0] == "#":
                continue
            images.append(line.split()[0])
    assert len(images) > 0
    return images


def parse_image_lists(paths):
    paths = Path(paths)
    files = list(Path(paths.parent).glob(paths.name))
    assert len(files) > 0
    images = []
    for lfile in files:
        images += parse_image_list(lfile)
    return images


def parse_names(prefix, names, names_all):
    if prefix is not None:
        if not isinstance(prefix, str):
            prefix = tuple(prefix)
        names = [n for n in names_all if n.startswith(prefix)]
        if len(names) == 0:
            raise ValueError(f"Could not find any image with the prefix `{prefix}`.")
    elif names is not None:
        if isinstance(names, (str, Path)):
            names = parse_image_lists(names)
        elif isinstance(names, collections.Iterable):
            names = list(names)
        else:
            raise ValueError(f"Unknown type of image list: {names}." "Provide either a list or a path to a list file.")
    else:
        names = names_all
    return names


def get_descriptors(names, path, name2idx=None, key="global_descriptor"):
    if name2idx is None:
        with open_h5(str(path), "r") as fd:
            desc = [fd[n][key].__array__() for n in names]
    else:
        desc = []
        for n in names:
            with open_h5(str(path[name2idx[n]]), "r") as fd:
                desc.append(fd[n][key].__array__())
    return torch.from_numpy(np.stack(desc, 0)).float()


def pairs_from_topk(indices: np.ndarray, values: np.ndarray) -> list:
    """The reference's walk over `np.where(valid)` (:66-70): (i, j) in row-major order of the [Q, num_select] ranks, non-finite ranks skipped."""
    valid = np.isfinite(values)
    return [(int(i), int(indices[i, j])) for i, j in zip(*np.where(valid))]


def topk_on_device(query_desc: torch.Tensor, db_desc: torch.Tensor, invalid: np.ndarray, num_select: int, min_score: Optional[float] = None, device="cuda"):
    """-> (indices, values) [Q, num_select] on the host; the similarity matrix stays on the device."""
    assert tuple(invalid.shape) == (query_desc.shape[0], db_desc.shape[0])
    idx, val = backend.retrieval_topk(query_desc.to(device), db_desc.to(device), num_select, torch.from_numpy(np.ascontiguousarray(invalid)), min_score)
    return idx.cpu().numpy(), val.cpu().numpy()


def pairs_from_score_matrix(scores: torch.Tensor, invalid: np.array, num_select: int, min_score: Optional[float] = None):
    """Reference signature (:50-71) for a score matrix the caller already holds: the mask, `min_score` and the top-k run on the device
    (scores times the identity), with the tie order of this module."""
    assert scores.shape == invalid.shape
    if isinstance(scores, np.ndarray):
        scores = torch.from_numpy(scores)
    dev = scores.device if scores.device.type == "cuda" else torch.device("cuda")
    eye = torch.eye(scores.shape[1], dtype=torch.float32, device=dev)
    idx, val = backend.retrieval_topk(scores.to(dev).float(), eye, num_select, torch.from_numpy(np.ascontiguousarray(invalid)), min_score)
    return pairs_from_topk(idx.cpu().numpy(), val.cpu().numpy())


def main(descriptors, output, num_matched, query_prefix=None, query_list=None, db_prefix=None, db_list=None, db_model=None, db_descriptors=None, device="cuda"):
    if db_model:
        raise NotImplementedError("pairs_from_retrieval: db_model (the image names of a COLMAP images.bin) is not served; pass db_list or db_prefix")
    # We handle multiple reference feature files.
    # We only assume that names are unique among them and map names to files.
    if db_descriptors is None:
        db_descriptors = descriptors
    if isinstance(db_descriptors, (Path, str)):
        db_descriptors = [db_descriptors]
    name2db = {n: i for i, p in enumerate(db_descriptors) for n in list_h5_names(p)}
    db_names_h5 = list(name2db.keys())
    query_names_h5 = list_h5_names(descriptors)

    db_names = parse_names(db_prefix, db_list, db_names_h5)
    if len(db_names) == 0:
        raise ValueError("Could not find any database image.")
    query_names = parse_names(query_prefix, query_list, query_names_h5)

    db_desc = get_descriptors(db_names, db_descriptors, name2db)
    query_desc = get_descriptors(query_names, descriptors)

    # Avoid self-matching
    self = np.array(query_names)[:, None] == np.array(db_names)[None]
    idx, val = topk_on_device(query_desc, db_desc, self, num_matched, min_score=0, device=device)
    pairs = [(query_names[i], db_names[j]) for i, j in pairs_from_topk(idx, val)]

    with open(output, "w") as f:
        f.write("\n".join(" ".join([i, j]) for i, j in pairs))
    return pairs


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--descriptors", type=Path, required=True)
    parser.add_argument("--output", type=Path, required=True)
    parser.add_argument("--num_matched", type=int, required=True)
    parser.add_argument("--query_prefix", type=str, nargs="+")
    parser.add_argument("--query_list", type=Path)
    parser.add_argument("--db_prefix", type=str, nargs="+")
    parser.add_argument("--db_list", type=Path)
    parser.add_argument("--db_model", type=Path)
    parser.add_argument("--db_descriptors", type=Path)
    args = parser.parse_args()
    main(**args.__dict__)
