"""Device-resident datasets: what feeds `DeviceAugmentation` / `RobustnessTest`.

The reference runs forward kinematics file by file as dozens of small torch ops (`utils/forward_kinematics.py::fkl_torch`,
`utils/ang2joint.py::ang2joint`), copies the result back, materialises every sliding window on the host
(`utils/data_utils.py::load_data_h36m` :843-942, `::load_data_amass` :738-839: `the_sequence[fs_sel]` - H3.6M training is 180 077
windows x 35 frames x 96 floats for ~50 MB of distinct frames), fixes inverted poses per window
(`loaders/h36m_motion_3d.py:70-74`) and ships every batch host -> device.  Here a `MotionBank` keeps the DISTINCT frames on the device
with a table of window starts; forward kinematics is one launch per file (`ops.forward_kinematics`) and a batch is cut by one gather
kernel (`ops.gather_windows`: joint selection, optional normalisation and the inversion fix included) straight into the `raw`
tensor the input pipeline takes.  With `batches(shuffle=True)` the permutation is drawn on the device: an epoch has no host batch
and no host -> device copy.

`h36m_bank` / `amass_bank` run the reference's file logic and then `MotionBank.from_sequences`.  The skeletons are arguments
(`tree=(parent, offset)` as `forward_kinematics._some_variables()` returns them; AMASS reads its own `smpl_skeleton.npz`), like
`dim_used` and `bones` elsewhere in this package.  `normalize` is false in every YAML of the reference: `mean` / `std` are taken as
scalars, the median / IQR statistics of `load_data_*` are not computed.
"""
import os

import numpy as np
import torch

from .. import ops

# load_data_h36m: subjects per split (data_utils.py:857) and the joints it drops (:920).  The two joints of the inversion check are an
# argument (`up_joints`): the reference takes the positions of the first "Head" and the first "Site" in the 32 joint names of
# body_utils.get_reduced_skeleton("h36m") - 14 and 5 - and indexes the 22 joints that stay with them (h36m_motion_3d.py:83-87).
H36M_SUBJECTS = {"train": (1, 6, 7, 8, 9), "test": (11, 5), "full_original_test": (5,), "original_test": (5,)}
H36M_IGNORED_JOINTS = (0, 1, 6, 11, 16, 20, 23, 24, 28, 31)
H36M_ACTIONS = ("walking", "eating", "smoking", "discussion", "directions", "greeting", "phoning", "posing", "purchases", "sitting",
                "sittingdown", "takingphoto", "waiting", "walkingdog", "walkingtogether")
AMASS_ACTIONS = ("HumanEva", "MPI_HDM05", "MPI_mosh", "SFU", "BioMotionLab_NTroje", "ACCAD", "CMU", "EKUT", "EyesJapanDataset", "KIT",
                 "MPI_Limits", "TCD_handMocap", "TotalCapture")
AMASS_SPLIT_FOLDERS = {"train": ("train",), "test": ("val", "test"), "original_test": ("test",)}


class MotionBank:
    """Distinct frames (F, J_src, 3) on the device and the first frame of every window.  Build one with `from_sequences`.

    frames      (F, J_src, 3) fp32 on the device, never written
    starts      (W,) int32 first frame of every window: `starts` a host numpy copy, `starts_dev` on the device
    labels      W strings (the reference's `class_seq`), `labels_of(items)` for `return_class`
    seq_len     frames per window;  select: joints a window keeps (the loaders' `dim_used`) or None
    mean, std   scalars of the optional normalisation (0 / 1: off);  up_joints: (head, hip) in the selected numbering for the
                pose-inversion fix, or None
    """

    def __init__(self, frames, starts, labels, seq_len, select=None, mean=0.0, std=1.0, up_joints=None):
        self.frames, self.seq_len = frames, int(seq_len)
        self.starts = np.ascontiguousarray(starts, dtype=np.int32)
        self.starts_dev = torch.from_numpy(self.starts).to(frames.device)
        self.labels = np.asarray(labels)
        self.select = None if select is None else [int(v) for v in select]
        self.mean, self.std = float(mean), float(std)
        self.up_joints = None if up_joints is None else (int(up_joints[0]), int(up_joints[1]))
        if len(self.labels) != len(self.starts):
            raise ValueError("MotionBank: %d labels for %d windows" % (len(self.labels), len(self.starts)))

    @classmethod
    def from_sequences(cls, seqs, labels, seq_len, skip_rate=1, starts=None, select=None, mean=0.0, std=1.0, up_joints=None):
        """seqs: (F_i, J, 3) fp32 device tensors, one per file; labels: one string per sequence.  Windows of `seq_len` frames
        start at `arange(0, F_i - seq_len + 1, skip_rate)` of every sequence, or at `starts[i]` (frame numbers inside sequence i)
        where `starts` is given.  Every start is checked here, on the host: a window never leaves its own sequence."""
        seq_len, skip_rate = int(seq_len), int(skip_rate)
        if seq_len < 1 or skip_rate < 1:
            raise ValueError("MotionBank: seq_len and skip_rate must be positive")
        if not seqs or len(labels) != len(seqs) or (starts is not None and len(starts) != len(seqs)):
            raise ValueError("MotionBank: need one label (and one start list) per sequence, and at least one sequence")
        all_starts, all_labels, base = [], [], 0
        for i, s in enumerate(seqs):
            ops._chk(s, "sequence %d" % i)
            if s.dim() != 3 or s.shape[2] != 3 or s.shape[1:] != seqs[0].shape[1:] or s.device != seqs[0].device:
                raise ValueError("MotionBank: sequence %d is %s on %s, expected (F, %d, 3) on %s"
                                 % (i, tuple(s.shape), s.device, seqs[0].shape[1], seqs[0].device))
            F = int(s.shape[0])
            st = np.arange(0, F - seq_len + 1, skip_rate, dtype=np.int64) if starts is None else np.asarray(starts[i], dtype=np.int64).reshape(-1)
            if st.size and (st.min() < 0 or st.max() + seq_len > F):
                raise ValueError("MotionBank: a window of %d frames starting at %d leaves sequence %d (%d frames)"
                                 % (seq_len, int(st.max() if st.max() + seq_len > F else st.min()), i, F))
            all_starts.append(st + base)
            all_labels += [labels[i]] * len(st)
            base += F
        if base >= 2 ** 31:
            raise ValueError("MotionBank: %d frames do not fit the int32 window table" % base)
        frames = seqs[0] if len(seqs) == 1 else torch.cat(list(seqs), 0)
        return cls(frames.contiguous(), np.concatenate(all_starts), all_labels, seq_len, select=select, mean=mean, std=std, up_joints=up_joints)

    def __len__(self):
        return int(self.starts.shape[0])

    @property
    def device(self):
        return self.frames.device

    def _host_items(self, items):
        ids = np.asarray(items.numpy() if torch.is_tensor(items) else items)
        if ids.size and not np.issubdtype(ids.dtype, np.integer):
            raise TypeError("MotionBank: window ids must be integers")
        ids = ids.astype(np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= len(self)):
            raise IndexError("MotionBank: window id %d out of range for %d windows" % (int(ids.max() if ids.max() >= len(self) else ids.min()), len(self)))
        return ids

    def windows(self, items):
        """raw (B, seq_len, J, 3) for the window ids `items`.  A host list / ndarray / CPU tensor is range-checked (IndexError) and
        uploaded; an integer tensor on the bank's device is trusted - the kernel clamps, nothing is read back."""
        if torch.is_tensor(items) and items.device == self.device:
            dev_items = items
        else:
            dev_items = torch.from_numpy(self._host_items(items).astype(np.int32)).to(self.device)
        return ops.gather_windows(self.frames, self.starts_dev, dev_items, self.seq_len, select=self.select, mean=self.mean, std=self.std,
                                  up_joints=self.up_joints)

    def labels_of(self, items):
        """the reference's `class_seq[item]` (`return_class`) for host or device ids"""
        return self.labels[self._host_items(items.cpu() if torch.is_tensor(items) else items)]

    def batches(self, batch_size, shuffle=False, drop_last=False, generator=None):
        """Yields {"raw": (b, seq_len, J, 3), "item": (b,) int32 on the device} over all windows once.  With `shuffle` the permutation
        is drawn on the device (`torch.randperm(..., device=...)`, `generator` a generator of that device): no host round trip."""
        batch_size, W = int(batch_size), len(self)
        if batch_size < 1:
            raise ValueError("MotionBank.batches: batch_size must be positive")
        if shuffle:
            order = torch.randperm(W, dtype=torch.int32, device=self.device, generator=generator)
        else:
            order = torch.arange(W, dtype=torch.int32, device=self.device)
        for at in range(0, W, batch_size):
            item = order[at:at + batch_size]
            if drop_last and item.shape[0] < batch_size:
                return
            yield {"raw": self.windows(item), "item": item}

    def feed(self, batch_size, shuffle=True, generator=None):
        """A `BankFeed`: the epoch's permutation and a cursor into it in static device buffers, for a step that gathers its own batch
        (`runtime.BankStep`)."""
        return BankFeed(self, batch_size, shuffle=shuffle, generator=generator)


class BankFeed:
    """The batches of a `MotionBank` epoch named on the device: `order` (W,) int32, the epoch's permutation of the window ids, and
    `cursor` (1,) int32, the position of the next batch in it.  Both are allocated once; `ops.gather_windows_at` reads them and
    `ops.cursor_advance` moves the cursor, so a captured step takes batch after batch without the host naming one.

    `len(feed)` = W // batch_size batches per epoch: the partial last batch is DROPPED (a captured step has one batch size).
    `start_epoch()` draws a new permutation into the same `order` buffer (`torch.randperm(device=...)`; `arange` without `shuffle`)
    and zeroes the cursor - no synchronisation, no reallocation.  `taken` counts, on the host, the batches taken since: the step
    that moves the cursor (`ops.cursor_advance`, or the replay of a graph that holds it) adds one."""

    def __init__(self, bank, batch_size, shuffle=True, generator=None):
        self.bank, self.batch_size, self.shuffle, self.generator = bank, int(batch_size), bool(shuffle), generator
        W = len(bank)
        if self.batch_size < 1 or self.batch_size > W:
            raise ValueError("BankFeed: batch_size %d for a bank of %d windows" % (self.batch_size, W))
        self.order = torch.empty(W, dtype=torch.int32, device=bank.device)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=bank.device)
        self.taken = 0
        self.start_epoch()

    def __len__(self):
        return len(self.bank) // self.batch_size

    def start_epoch(self):
        W = len(self.bank)
        if self.shuffle:
            self.order.copy_(torch.randperm(W, dtype=torch.int32, device=self.bank.device, generator=self.generator))
        else:
            self.order.copy_(torch.arange(W, dtype=torch.int32, device=self.bank.device))
        self.cursor.zero_()
        self.taken = 0
        return self

    def items(self):
        """the window ids of the batch the next step takes: a view of `order` (for `MotionBank.labels_of`)"""
        at = self.taken * self.batch_size
        return self.order[at:at + self.batch_size]

    def gather(self, out=None):
        """raw (batch_size, seq_len, J, 3) of the batch at the cursor (`ops.gather_windows_at`); the cursor is not moved"""
        b = self.bank
        return ops.gather_windows_at(b.frames, b.starts_dev, self.order, self.cursor, self.batch_size, b.seq_len, select=b.select, mean=b.mean,
                                     std=b.std, up_joints=b.up_joints, out=out)


def find_indices_256(frame_num1, frame_num2, seq_len, input_n=10):
    """First frames of the 2 x 128 evaluation windows of the `original_test` split (data_utils.py:77-106): RandomState(1234567890),
    alternating `randint(16, F - 150)` for the two sub-actions, start = draw + 50 - input_n.  Returns two (128,) arrays."""
    rng = np.random.RandomState(1234567890)
    s1, s2 = [], []
    for _ in range(128):
        s1.append(rng.randint(16, frame_num1 - 150) + 50 - input_n)
        s2.append(rng.randint(16, frame_num2 - 150) + 50 - input_n)
    return np.asarray(s1, dtype=np.int64), np.asarray(s2, dtype=np.int64)


def _actions(actions, known, what):
    if isinstance(actions, (list, tuple)) and len(actions) == 1:
        actions = actions[0]
    if isinstance(actions, str):
        if actions == "all":
            return list(known)
        if actions == "all_srnn" and what == "H3.6M":
            return ["walking", "eating", "smoking", "discussion"]
        if actions in known:
            return [actions]
        raise ValueError("unrecognized %s action: %r" % (what, actions))
    return list(actions)


def _read_csv(path):
    """`readCSVasFloat` (data_utils.py:295-315): comma-separated floats, one frame per line"""
    with open(path) as f:
        rows = [np.array(line.strip().split(","), dtype=np.float32) for line in f if line.strip()]
    return np.stack(rows)


def h36m_bank(path, actions, input_n, output_n, split, tree, dim_used=None, up_joints=None, device="cuda", mean=0.0, std=1.0):
    """`load_data_h36m` + `H36m_Motion3D.__init__` as a bank.  path: the folder that holds `S1/`, `S5/`, ... (the reference's
    `<path_to_data>/dataset`); actions: a name, "all", "all_srnn" or a list; split: train / test / full_original_test /
    original_test; tree = (parent, offset): the 32-joint skeleton as `forward_kinematics._some_variables()` gives it (offset (32,3)).
    Per file: parse, zero columns 0:6, keep every second frame (before the kinematics - they are per frame), chain forward kinematics
    on the device, all windows at stride 1 (`original_test`: the 2 x 128 windows of `find_indices_256`).  dim_used: joints a window
    keeps (default: the loader's 22); up_joints: (head, hip) in that numbering for the inversion fix, None: off."""
    if split not in H36M_SUBJECTS:
        raise ValueError("h36m_bank: split must be one of %s" % ", ".join(H36M_SUBJECTS))
    parent, offset = tree
    offset = np.asarray(offset, dtype=np.float32).reshape(-1, 3)
    seq_len = int(input_n) + int(output_n)
    if dim_used is None:
        dim_used = [j for j in range(offset.shape[0]) if j not in H36M_IGNORED_JOINTS]
    rest = torch.from_numpy(offset).to(device)
    seqs, labels, starts = [], [], []
    for action in _actions(actions, H36M_ACTIONS, "H3.6M"):
        for subj in H36M_SUBJECTS[split]:
            pair = []
            for subact in (1, 2):
                a = _read_csv(os.path.join(str(path), "S%d" % subj, "%s_%d.txt" % (action, subact)))
                a[:, 0:6] = 0
                a = np.ascontiguousarray(a[::2])
                pair.append(ops.forward_kinematics(torch.from_numpy(a).to(device), parent, rest, convention="expmap_chain"))
            seqs += pair
            labels += [action, action]
            if split == "original_test":
                starts += list(find_indices_256(pair[0].shape[0], pair[1].shape[0], seq_len, input_n=int(input_n)))
    return MotionBank.from_sequences(seqs, labels, seq_len, starts=starts if split == "original_test" else None, select=dim_used,
                                     mean=mean, std=std, up_joints=up_joints)


def amass_bank(path, actions, input_n, output_n, split, dim_used=None, device="cuda", mean=0.0, std=1.0, skip_rate=5):
    """`load_data_amass` + `Amass_Motion3D.__init__` as a bank.  path holds `smpl_skeleton.npz` (`p3d0` (1,J,3), `parents` (J,)) and the
    split folders (train | val + test | test); every `*.npz` below them whose path contains one of the action strings is read (in
    sorted order per folder; the reference takes the order of the directory scan), files without `poses` are skipped.  Per file:
    every `int(mocap_framerate // 25)`-th frame, root pose zeroed, SMPL forward kinematics x 1000 on the device, the first 22 joints,
    windows every `skip_rate` frames.  dim_used defaults to joints 4 .. 21.  Labels are `<folder>_<file>` as in the reference."""
    if split not in AMASS_SPLIT_FOLDERS:
        raise ValueError("amass_bank: split must be one of %s" % ", ".join(AMASS_SPLIT_FOLDERS))
    from pathlib import Path
    path = Path(path)
    skel = np.load(path / "smpl_skeleton.npz")
    p3d0 = np.asarray(skel["p3d0"], dtype=np.float32).reshape(-1, 3)
    parent = [int(v) for v in skel["parents"]]
    parent[0] = -1
    rest = torch.from_numpy(p3d0[:len(parent)].copy()).to(device)
    used = list(range(min(22, len(parent))))
    if dim_used is None:
        dim_used = list(range(4, 22))
    seq_len = int(input_n) + int(output_n)
    files = [f for folder in AMASS_SPLIT_FOLDERS[split] for f in sorted((path / folder).rglob("*.npz"))]
    files = [f for a in _actions(actions, AMASS_ACTIONS, "AMASS") for f in files if a in str(f)]
    seqs, labels = [], []
    for f in files:
        rec = np.load(f)
        if "poses" not in rec.files:
            continue
        poses = rec["poses"]
        rate = int(rec["mocap_framerate"] // 25)
        poses = np.ascontiguousarray(poses[::rate], dtype=np.float32).reshape(-1, poses.shape[1] // 3, 3)
        poses[:, 0] = 0
        seqs.append(ops.forward_kinematics(torch.from_numpy(poses).to(device), parent, rest, convention="smpl", select=used, scale=1000.0))
        labels.append(f.parent.stem + "_" + f.stem)
    if not seqs:
        raise FileNotFoundError("amass_bank: no usable *.npz for %r under %s" % (actions, path))
    return MotionBank.from_sequences(seqs, labels, seq_len, skip_rate=skip_rate, select=dim_used, mean=mean, std=std)
