"""Model of the host-fed stream's ring (include/aruco_slam_hip.h, "host-fed stream") in plain Python: which frame goes to which slot in
which submit.  It knows nothing of the library.  The rules, as the header states them:
 * the ring has two halves of H slots; frame k of a half lands in slot half * H + k;
 * a half is submitted when it holds H frames, or at a flush if it holds at least one; a submit moves on to the other half;
 * a flush of an empty half submits nothing and stays on its half;
 * opening the stream again first submits what is committed, as a flush does, and then starts at half 0 with the new H; what the
   slots held before stays in them until a later submit overwrites it.
A frame is counted when it is committed (a push, or an acquire + commit); frames are numbered 0, 1, ... in that order."""

OVERWRITTEN = "overwritten"
PENDING = "pending"


class Ring:
    def __init__(self, H):
        self.H, self.half, self.pending = H, 0, []
        self.submits = []          # per submit: (half, slot0, n, [frame indices])
        self.slot_of = []          # per frame: its slot, PENDING before its submit, OVERWRITTEN once another frame took the slot
        self.frame_in = {}         # per slot that was ever written: the frame it holds now

    def next_slot(self):
        """where the next committed frame will land"""
        return self.half * self.H + len(self.pending)

    def _submit(self):
        if not self.pending:
            return None
        slot0 = self.half * self.H
        for k, f in enumerate(self.pending):
            if slot0 + k in self.frame_in:
                self.slot_of[self.frame_in[slot0 + k]] = OVERWRITTEN
            self.frame_in[slot0 + k] = f
            self.slot_of[f] = slot0 + k
        s = (self.half, slot0, len(self.pending), self.pending)
        self.submits.append(s)
        self.half ^= 1
        self.pending = []
        return s

    def commit(self):
        """one frame committed; returns the submit it completes, or None"""
        self.pending.append(len(self.slot_of))
        self.slot_of.append(PENDING)
        return self._submit() if len(self.pending) == self.H else None

    push = commit

    def flush(self):
        return self._submit()

    def open(self, H):
        s = self._submit()
        self.H, self.half = H, 0
        return s


def run(ops, H):
    """ops: "push" / "commit" / "flush" / ("open", H).  Returns (submits, slot_of) after the last operation."""
    r = Ring(H)
    for op in ops:
        if op in ("push", "commit"):
            r.commit()
        elif op == "flush":
            r.flush()
        else:
            r.open(op[1])
    return r.submits, r.slot_of
