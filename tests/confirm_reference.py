"""Landmark confirmation (include/aruco_slam_hip.h) restated in plain Python; a helper module.

One ConfirmTable per SLAM filter.  judge(ids, valid) is one EKF slot: it returns the valid flags the slot's list is left with and the
slot's record, and moves the table on."""
ID_TABLE = 1024
LIST_MAX = 128


class ConfirmTable:
    def __init__(self, min_sightings, max_gap, confirmed=()):
        self.K, self.G = int(min_sightings), int(max_gap)
        self.reseed(confirmed)

    def reseed(self, landmark_ids=()):
        self.confirmed = {int(i) for i in landmark_ids if 0 <= int(i) < ID_TABLE}
        self.count, self.last, self.t = {}, {}, 0

    def judge(self, ids, valid):
        ids, out = [int(i) for i in ids][:LIST_MAX], [int(v) for v in valid]
        self.t += 1
        judged = [k for k, i in enumerate(ids) if out[k] != 0 and 0 <= i < ID_TABLE]
        U = sorted({ids[k] for k in judged} - self.confirmed)
        promoted = 0
        for i in U:                                               # step A
            if self.count.get(i, 0) > 0 and self.t - self.last[i] > self.G:
                self.count[i] = 0
            self.count[i] = self.count.get(i, 0) + 1
            self.last[i] = self.t
            if self.count[i] >= self.K:
                self.confirmed.add(i)
                self.count[i] = 0
                promoted += 1
        mask = [0, 0, 0, 0]
        withheld = [k for k in judged if ids[k] not in self.confirmed]
        for k in withheld:                                        # step B
            out[k] = 0
            mask[k // 32] |= 1 << (k % 32)
        return out, dict(judged=len(judged), tentative=len(U), withheld=len(withheld), promoted=promoted, withheld_mask=mask)

    def tentative(self):
        """(ids, counts, ages), ascending by id"""
        live = [i for i in sorted(self.count) if self.count[i] > 0 and self.t - self.last[i] <= self.G]
        return live, [self.count[i] for i in live], [self.t - self.last[i] for i in live]
