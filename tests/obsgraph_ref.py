"""Plain-Python restatement of the reference's observation table and the four loops over it, with dicts keyed by mnId.
The reference iterates std::map<KeyFrame*, ...> in pointer order; here every such map is walked in ascending mnId, the
order include/orbfe.h defines for the device table.  The float part uses numpy float32 / float64 exactly as the header
spells it out.  Nothing here touches the library under test."""
import numpy as np

f32, f64 = np.float32, np.float64


class World:
    """Key frames {id: dict(Ow, bad)} and points {pid: dict(obs {kf id: (idx, octave, stereo)}, nObs, bad, ref)}."""

    def __init__(self):
        self.kfs, self.pts = {}, {}

    def add_keyframe(self, kid, Ow, bad=False):
        self.kfs[kid] = {"Ow": np.asarray(Ow, f32), "bad": bool(bad)}

    def add_point(self, pid, ref=-1, bad=False):
        self.pts[pid] = {"obs": {}, "nObs": 0, "bad": bool(bad), "ref": ref}

    # MapPoint::AddObservation, src/MapPoint.cc:101-114
    def add_observation(self, pid, kid, idx, octave, stereo):
        p = self.pts[pid]
        if kid in p["obs"]:
            return
        p["obs"][kid] = (int(idx), int(octave), bool(stereo))
        p["nObs"] += 2 if stereo else 1

    # MapPoint::EraseObservation :119-145 with SetBadFlag :164-182 -> True when the point became bad
    def erase_observation(self, pid, kid):
        p = self.pts[pid]
        if kid not in p["obs"]:
            return False
        p["nObs"] -= 2 if p["obs"][kid][2] else 1
        del p["obs"][kid]
        if p["ref"] == kid:
            p["ref"] = min(p["obs"]) if p["obs"] else -1  # mObservations.begin()->first
        if p["nObs"] <= 2:
            p["bad"] = True
            p["obs"] = {}
            return True
        return False

    # the map-point part of KeyFrame::SetBadFlag, src/KeyFrame.cc:488 ff. -> the points that became bad, ascending
    def erase_keyframe(self, kid):
        out = [pid for pid in sorted(self.pts) if kid in self.pts[pid]["obs"] and self.erase_observation(pid, kid)]
        self.kfs[kid]["bad"] = True
        return out

    # the counting loops of KeyFrame::UpdateConnections (src/KeyFrame.cc:326-344; self_id = mnId) and of
    # Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1346-1362; self_id = None) -> {kf id: votes}
    def votes(self, pids, self_id=None):
        counter = {}
        for pid in pids:
            p = self.pts[pid]
            if p["bad"]:
                continue
            for kid in sorted(p["obs"]):
                if kid == self_id:
                    continue
                counter[kid] = counter.get(kid, 0) + 1
        return counter

    # LocalMapping::KeyFrameCulling, src/LocalMapping.cc:725-769, for one candidate -> (nMPs, nRedundantObservations)
    def culling_counts(self, kid, features):
        n_mps = n_red = 0
        for pid, level in features:
            p = self.pts[pid]
            if p["bad"]:
                continue
            n_mps += 1
            if p["nObs"] > 3:
                n = 0
                for ki in sorted(p["obs"]):
                    if ki == kid:
                        continue
                    if p["obs"][ki][1] <= level + 1:
                        n += 1
                        if n >= 3:
                            break
                if n >= 3:
                    n_red += 1
        return n_mps, n_red

    # the whole of KeyFrameCulling :718-773 over candidates [(kf id, features)] -> (culled ids, points that became bad)
    def keyframe_culling(self, candidates):
        culled, bad = [], []
        for kid, features in candidates:
            n_mps, n_red = self.culling_counts(kid, features)
            if should_cull(n_mps, n_red):
                culled.append(kid)
                bad += self.erase_keyframe(kid)
        return culled, bad

    # MapPoint::UpdateNormalAndDepth, src/MapPoint.cc:360-404 -> (normal, min, max) or None where it returns early
    def normal_depth(self, pid, pos, scale_factors):
        p = self.pts[pid]
        if p["bad"] or not p["obs"] or p["ref"] not in p["obs"]:
            return None
        P = np.asarray(pos, f32)
        normal = np.zeros(3, f32)
        n = 0
        for kid in sorted(p["obs"]):
            d = (P - self.kfs[kid]["Ow"]).astype(f32)
            nrm = np.sqrt(f64(d[0]) * f64(d[0]) + f64(d[1]) * f64(d[1]) + f64(d[2]) * f64(d[2]))
            a = f32(f64(1.0) / nrm)
            normal = (normal + (d * a).astype(f32)).astype(f32)
            n += 1
        normal = (normal * f32(f64(1.0) / f64(n))).astype(f32)
        pc = (P - self.kfs[p["ref"]]["Ow"]).astype(f32)
        dist = f32(np.sqrt(f64(pc[0]) * f64(pc[0]) + f64(pc[1]) * f64(pc[1]) + f64(pc[2]) * f64(pc[2])))
        sf = np.asarray(scale_factors, f32)
        hi = f32(dist * sf[p["obs"][p["ref"]][1]])
        lo = f32(hi / sf[len(sf) - 1])
        return normal, lo, hi


def should_cull(n_mps, n_red):
    """nRedundantObservations > 0.9 * nMPs: int against double (src/LocalMapping.cc:771)."""
    return float(n_red) > 0.9 * float(n_mps)


# KeyFrame::UpdateConnections :347-393 on KFcounter {id: weight}
def update_connections(counter, th=15):
    if not counter:
        return {"ordered_id": [], "ordered_weight": [], "connect_id": [], "connect_weight": [], "parent_id": -1}
    nmax, kfmax, pairs, connect = 0, None, [], []
    for kid in sorted(counter):
        w = counter[kid]
        if w > nmax:
            nmax, kfmax = w, kid
        if w >= th:
            pairs.append((w, kid))
            connect.append((kid, w))
    if not pairs:
        pairs.append((nmax, kfmax))
        connect.append((kfmax, nmax))
    pairs.sort()
    ordered = pairs[::-1]  # push_front
    return {"ordered_id": [k for _, k in ordered], "ordered_weight": [w for w, _ in ordered],
            "connect_id": [k for k, _ in connect], "connect_weight": [w for _, w in connect], "parent_id": ordered[0][1]}


# Tracking::UpdateLocalKeyFrames :1364-1454 on keyframeCounter {id: weight}
def local_keyframes(counter, bad, neighbours, children, parent):
    if not counter:
        return [], -1
    local, tracked, best, ref = [], set(), 0, -1
    for kid in sorted(counter):
        if kid in bad:
            continue
        if counter[kid] > best:
            best, ref = counter[kid], kid
        local.append(kid)
        tracked.add(kid)
    for kid in list(local):  # the end iterator is taken before the vector grows (:1393)
        if len(local) > 80:
            break
        for nb in neighbours.get(kid, [])[:10]:
            if nb not in bad and nb not in tracked:
                local.append(nb)
                tracked.add(nb)
                break
        for ch in sorted(children.get(kid, [])):
            if ch not in bad and ch not in tracked:
                local.append(ch)
                tracked.add(ch)
                break
        par = parent.get(kid, -1)
        if par >= 0 and par not in tracked:
            local.append(par)
            tracked.add(par)
            break
    return local, ref


def load(world, graph, kf_slot_of, slot_of):
    """Writes `world` into an ObservationGraph: kf id -> kf slot and point id -> slot by the two dicts."""
    ids = sorted(world.kfs)
    graph.set_keyframes([kf_slot_of[k] for k in ids], ids, [world.kfs[k]["Ow"] for k in ids], [world.kfs[k]["bad"] for k in ids])
    pids = sorted(world.pts)
    graph.set_points([slot_of[p] for p in pids], [world.pts[p]["bad"] for p in pids],
                     [kf_slot_of.get(world.pts[p]["ref"], -1) for p in pids])
    rows = [(slot_of[p], kf_slot_of[k], *world.pts[p]["obs"][k]) for p in pids for k in world.pts[p]["obs"]]
    if rows:
        graph.add_observations(*[list(c) for c in zip(*rows)])


def mirror_row(world, pid, kf_slot_of):
    """What get_row must return for point `pid`: entries in ascending mnId."""
    p = world.pts[pid]
    ent = [(kf_slot_of[k], p["obs"][k][0], p["obs"][k][1], 1 if p["obs"][k][2] else 0) for k in sorted(p["obs"])]
    return ent, p["nObs"], int(p["bad"]), kf_slot_of.get(p["ref"], -1)
