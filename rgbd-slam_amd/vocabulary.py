"""The DBoW3 vocabulary as arrays (the form rgbd_voc_set takes) and its text YAML file.

Vocabulary holds one row per node, node 0 the root: parent, descriptor (32 bytes), weight, is_leaf and, on leaves,
word_id.  The children of a node are ordered by node id, which is the order DBoW3 keeps them in.

load_dbow3_yaml / save_dbow3_yaml read and write DBoW3's text YAML (Vocabulary::save / load over cv::FileStorage),
plain or gzip-compressed by the file name's .gz.  DBoW3 is not available to this project: the layout below is
RECALLED from the library's source and is UNPINNED against a file the library wrote.

    %YAML:1.0
    ---
    vocabulary:
       k: 10
       L: 6
       scoringType: 0
       weightingType: 0
       nodes:
          - { nodeId:1, parentId:0, weight:0., descriptor:"dbw3 0 32 b0 b1 ... b31" }
       words:
          - { wordId:0, nodeId:19 }

The root (node 0) has no `nodes` entry; a descriptor string is "dbw3 <cv type> <cols>" followed by the bytes in
decimal (cv type 0 = CV_8U).  A node is a leaf when a `words` entry names it.  Weights are written with repr(), so
a round trip through this module keeps every bit; a file from the library carries the digits cv::FileStorage chose.
"""
from __future__ import annotations

import gzip
import re
from dataclasses import dataclass

import numpy as np

TF_IDF, TF, IDF, BINARY = range(4)                                             # DBoW3::WeightingType
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)        # DBoW3::ScoringType


@dataclass
class Vocabulary:
    k: int
    L: int
    parent: np.ndarray       # (N,) i32; parent[0] is unused
    descriptor: np.ndarray   # (N, 32) u8
    weight: np.ndarray       # (N,) f64
    is_leaf: np.ndarray      # (N,) u8
    word_id: np.ndarray      # (N,) i32; -1 on inner nodes
    weighting: int = TF_IDF
    scoring: int = L1_NORM

    def __post_init__(self):
        self.parent = np.ascontiguousarray(self.parent, np.int32)
        self.descriptor = np.ascontiguousarray(self.descriptor, np.uint8)
        self.weight = np.ascontiguousarray(self.weight, np.float64)
        self.is_leaf = np.ascontiguousarray(self.is_leaf, np.uint8)
        self.word_id = np.ascontiguousarray(self.word_id, np.int32)

    @property
    def n_nodes(self) -> int:
        return len(self.parent)

    @property
    def n_words(self) -> int:
        return int(self.is_leaf.sum())

    def children(self):
        """Per node, its children in node-id order."""
        out = [[] for _ in range(self.n_nodes)]
        for i in range(1, self.n_nodes):
            out[int(self.parent[i])].append(i)
        return out

    def equal(self, o: "Vocabulary") -> bool:
        return (self.k, self.L, self.weighting, self.scoring) == (o.k, o.L, o.weighting, o.scoring) and all(
            np.array_equal(a, b) for a, b in ((self.parent[1:], o.parent[1:]), (self.descriptor[1:], o.descriptor[1:]),
                                              (self.weight[1:].view(np.uint64), o.weight[1:].view(np.uint64)),
                                              (self.is_leaf, o.is_leaf), (self.word_id, o.word_id)))


def _open(path, mode):
    return gzip.open(path, mode + "t") if str(path).endswith(".gz") else open(path, mode)


def save_dbow3_yaml(voc: Vocabulary, path) -> None:
    with _open(path, "w") as f:
        f.write("%YAML:1.0\n---\nvocabulary:\n")
        f.write(f"   k: {voc.k}\n   L: {voc.L}\n   scoringType: {voc.scoring}\n   weightingType: {voc.weighting}\n")
        f.write("   nodes:\n")
        for i in range(1, voc.n_nodes):
            d = " ".join(str(int(b)) for b in voc.descriptor[i])
            f.write(f"      - {{ nodeId:{i}, parentId:{int(voc.parent[i])}, weight:{float(voc.weight[i])!r},\n"
                    f"          descriptor:\"dbw3 0 {voc.descriptor.shape[1]} {d} \" }}\n")
        f.write("   words:\n")
        for i in np.flatnonzero(voc.is_leaf):
            f.write(f"      - {{ wordId:{int(voc.word_id[i])}, nodeId:{int(i)} }}\n")


_NODE = re.compile(r"nodeId\s*:\s*(\d+)\s*,\s*parentId\s*:\s*(\d+)\s*,\s*weight\s*:\s*([^,\s]+)\s*,\s*"
                   r"descriptor\s*:\s*\"dbw3\s+(\d+)\s+(\d+)\s+([\d\s]*)\"", re.S)
_WORD = re.compile(r"wordId\s*:\s*(\d+)\s*,\s*nodeId\s*:\s*(\d+)")


def load_dbow3_yaml(path) -> Vocabulary:
    with _open(path, "r") as f:
        text = f.read()
    head = {}
    for key in ("k", "L", "scoringType", "weightingType"):
        m = re.search(rf"^\s*{key}\s*:\s*(-?\d+)\s*$", text, re.M)
        if not m:
            raise ValueError(f"{path}: no '{key}' in the vocabulary")
        head[key] = int(m.group(1))
    cut = text.find("words:")
    if cut < 0 or "nodes:" not in text[:cut]:
        raise ValueError(f"{path}: no nodes / words lists")
    nodes = _NODE.findall(text[:cut])
    words = _WORD.findall(text[cut:])
    n = 1 + max((int(t[0]) for t in nodes), default=0)
    if len(nodes) != n - 1:
        raise ValueError(f"{path}: node ids are not 1 .. {n - 1}, once each")
    parent, weight = np.zeros(n, np.int32), np.zeros(n, np.float64)
    desc = np.zeros((n, 32), np.uint8)
    for nid, pid, w, ctype, cols, data in nodes:
        i = int(nid)
        b = [int(x) for x in data.split()]
        if int(ctype) != 0 or int(cols) != 32 or len(b) != 32:
            raise ValueError(f"{path}: node {i}: not a 32-byte CV_8U descriptor")
        parent[i], weight[i], desc[i] = int(pid), float(w), b
    leaf, word = np.zeros(n, np.uint8), np.full(n, -1, np.int32)
    for wid, nid in words:
        leaf[int(nid)], word[int(nid)] = 1, int(wid)
    return Vocabulary(head["k"], head["L"], parent, desc, weight, leaf, word, head["weightingType"], head["scoringType"])
