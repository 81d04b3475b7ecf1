"""A restatement, in plain Python lists and sets, of the reference's loops over ``KeyFrame::mvpMapPoints``: the ordered union
that appears four times (Tracking::UpdateLocalPoints, LocalMapping::SearchInNeighbors, LoopClosing::ComputeSim3 and the
lLocalMapPoints of Optimizer::LocalBundleAdjustment) and KeyFrame::TrackedMapPoints.  What the device rows of the
observation graph (orbfe_obsgraph_keyframe_points_union / _tracked_points) are pinned against.

A point is a slot number; ``None`` in a row is a NULL pointer.  ``bad`` is the set of slots whose ``isBad()`` is true -- a slot
the graph was never told about counts as bad there, so the tests put such slots into ``bad`` as well."""


class KeyFramePoints:
    """rows: {kf: [slot or None, ...]} = mvpMapPoints per key frame; bad: set of slots; n_obs: {slot: MapPoint::nObs}."""

    def __init__(self):
        self.rows = {}
        self.bad = set()
        self.n_obs = {}

    # ---- mutations (src/KeyFrame.cc:220-243) ----
    def set_row(self, kf, slots):
        self.rows[kf] = [None if s is None or s < 0 else int(s) for s in slots]  # KeyFrame::KeyFrame: mvpMapPoints(F.mvpMapPoints) (:42)

    def assign(self, kf, idx, slot):
        self.rows[kf][idx] = None if slot is None or slot < 0 else int(slot)  # AddMapPoint :223, ReplaceMapPointMatch :242, EraseMapPointMatch :229

    # ---- the four loops ----
    def _union(self, kfs):
        out, stamped = [], set()
        for kf in kfs:                      # src/Tracking.cc:1315  itKF over mvpLocalKeyFrames, in order
            for p in self.rows[kf]:         # :1318-1320           GetMapPointMatches(), in idx order
                if p is None:               # :1323                if(!pMP) continue
                    continue
                if p in stamped:            # :1325                mnTrackReferenceForFrame == mCurrentFrame.mnId: continue
                    continue
                if p not in self.bad:       # :1327                if(!pMP->isBad())
                    out.append(p)           # :1329                push_back
                    stamped.add(p)          # :1330                the stamp
        return out

    def local_points(self, local_keyframes):
        """Tracking::UpdateLocalPoints, src/Tracking.cc:1315-1333."""
        return self._union(local_keyframes)

    def fuse_candidates(self, target_keyframes):
        """LocalMapping::SearchInNeighbors, src/LocalMapping.cc:555-571: if(!pMP) continue (:564); isBad() ||
        mnFuseCandidateForKF == current (:566) continue; stamp (:568), push_back (:569) -- the same loop."""
        return self._union(target_keyframes)

    def loop_points(self, loop_connected_keyframes):
        """LoopClosing::ComputeSim3, src/LoopClosing.cc:420-436: if(pMP) (:427), !isBad() && mnLoopPointForKF != current
        (:429), push_back (:431), stamp (:432) -- the same loop; the caller appends mpMatchedKF to the list (:418)."""
        return self._union(loop_connected_keyframes)

    def local_ba_points(self, local_keyframes):
        """lLocalMapPoints of Optimizer::LocalBundleAdjustment, src/Optimizer.cc:503-518: over lLocalKeyFrames, if(pMP) if(!pMP->isBad())
        if(mnBALocalForKF != pKF->mnId) push_back and stamp -- the same loop."""
        return self._union(local_keyframes)

    def tracked_points(self, kf, min_obs):
        """KeyFrame::TrackedMapPoints, src/KeyFrame.cc:264-289."""
        n = 0
        check = min_obs > 0                          # :269 bCheckObs
        for p in self.rows[kf]:                      # :270
            if p is None:                            # :273 if(pMP)
                continue
            if p in self.bad:                        # :275 if(!pMP->isBad())
                continue
            if check:
                if self.n_obs.get(p, 0) >= min_obs:  # :279 Observations() >= minObs
                    n += 1
            else:
                n += 1                               # :283
        return n
