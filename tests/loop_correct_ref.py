"""Plain-numpy restatement of the head of LoopClosing::CorrectLoop (src/LoopClosing.cc:514-604) and of the map update at the
tail of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:787-852), written as the reference's sequential loops:
a per-key-frame camera centre that changes at the reference's SetPose, a per-point flag that is set when the point is
corrected.  Sim3 maps come from essgraph_ref, the per-point normal / range from obsgraph_ref.World.normal_depth with the
centres current at that moment.  The std::map<KeyFrame*, ..> of :558 is walked in the order the caller gives.

Float cv::Mat products follow include/orbfe.h: cv::gemm on CV_32F accumulates in double, `R * P + t` is one gemm with
beta = 1: D_ij = float32(sum_k float64(A_ik) * float64(B_kj) [+ float64(C_ij)]), added left to right.
Nothing here touches the library under test."""
import numpy as np

import essgraph_ref as er

f32, f64 = np.float32, np.float64


def mul44(A, B):
    A, B = np.asarray(A, f32).reshape(4, 4), np.asarray(B, f32).reshape(4, 4)
    D = np.zeros((4, 4), f32)
    for i in range(4):
        for j in range(4):
            s = f64(A[i, 0]) * f64(B[0, j])
            for k in (1, 2, 3):
                s = s + f64(A[i, k]) * f64(B[k, j])
            D[i, j] = f32(s)
    return D


def rigid_map(T, X):
    T = np.asarray(T, f32).reshape(4, 4)
    out = np.zeros(3, f32)
    for i in range(3):
        s = f64(T[i, 0]) * f64(X[0])
        s = s + f64(T[i, 1]) * f64(X[1])
        s = s + f64(T[i, 2]) * f64(X[2])
        s = s + f64(T[i, 3])
        out[i] = f32(s)
    return out


def sim3_of_pose(T):
    """g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0) (:539-541, :547-549)"""
    T = np.asarray(T, f32).reshape(4, 4)
    return er.sim3_from_Rts(T[:3, :3].astype(f64), T[:3, 3].astype(f64), 1.0)


def correct_loop_sim3s(Tiw, Twc_cur, cur, Scw):
    """(:519-551, :590-596) -> (corrected [K, 8], noncorrected [K, 8], Tiw_corrected [K, 4, 4])"""
    scw = er.from_record(np.asarray(Scw, f64))
    cor, non, out = [], [], []
    for k, T in enumerate(np.asarray(Tiw, f32).reshape(-1, 4, 4)):
        if k == cur:
            S = scw  # CorrectedSim3[mpCurrentKF] = mg2oScw (:519)
        else:
            Tic = mul44(T, Twc_cur)  # (:538)
            S = er.sim3_mul(sim3_of_pose(Tic), scw)  # (:541-542)
        cor.append(er.to_record(S))
        non.append(er.to_record(sim3_of_pose(T)))  # (:547-551)
        out.append(er.tiw(S))  # (:590-596)
    return np.array(cor), np.array(non), np.array(out, f32)


def correct_point(cor, non, P):
    """g2oCorrectedSwi.map(g2oSiw.map(eigP3Dw)) (:578-583), stored as float"""
    Y = er.sim3_map(er.from_record(non), np.asarray(P, f32).astype(f64))
    return er.sim3_map(er.sim3_inverse(er.from_record(cor)), Y).astype(f32)


def correct_loop(world, order, rows, corrected, noncorrected, Ow_corrected, pos, skip, scale_factors):
    """The loop of :558-604.  world: obsgraph_ref.World, its key frames' Ow are REWRITTEN as the loop calls SetPose; order:
    the kf ids in visiting order; rows {kf id: [point id or -1]} = mvpMapPoints; pos {point id: float32[3]}, rewritten;
    skip: the point ids with mnCorrectedByKF == current -> (ids, refs, valid, {point id: (normal, min, max)})."""
    done, seen = set(skip), set()
    ids, refs, valid, nd = [], [], [], {}
    for k, kid in enumerate(order):
        if kid in seen:  # a std::map holds a key frame once
            continue
        seen.add(kid)
        for pid in rows[kid]:
            if pid < 0:  # !pMPi (:570)
                continue
            if pid not in world.pts or world.pts[pid]["bad"]:  # isBad() (:572)
                continue
            if pid in done:  # mnCorrectedByKF == mpCurrentKF->mnId (:574)
                continue
            pos[pid] = correct_point(corrected[k], noncorrected[k], pos[pid])
            done.add(pid)  # (:584)
            ids.append(pid)
            refs.append(k)  # mnCorrectedReference (:585)
            r = world.normal_depth(pid, pos[pid], scale_factors)  # (:586): with the centres as they are NOW
            valid.append(int(r is not None))
            if r is not None:
                nd[pid] = r
        world.kfs[kid]["Ow"] = np.asarray(Ow_corrected[k], f32)  # SetPose (:600)
    return ids, refs, valid, nd


def correct_loop_points(corrected, noncorrected, kf_points, xw, skip=None):
    """The same loop on arrays, without normal / range -> (xw_out, corrected_ref)"""
    out = np.asarray(xw, f32).copy()
    ref = np.full(len(out), -1, np.int32)
    for k, lst in enumerate(kf_points):
        for p in lst:
            if p < 0 or (skip is not None and skip[p]) or ref[p] >= 0:
                continue
            out[p] = correct_point(corrected[k], noncorrected[k], xw[p])
            ref[p] = k
    return out, ref


def gba_propagate_keyframes(origins, children, Tcw, Twc, in_gba, Tcw_gba):
    """(:788-815) -> (Tcw_new, reached, visited); ValueError where a key frame enters the list twice"""
    n = len(Tcw)
    T = [np.asarray(t, f32).reshape(4, 4).copy() for t in Tcw_gba]  # mTcwGBA
    flag = [bool(x) for x in in_gba]  # mnBAGlobalForKF == nLoopKF
    visited = [False] * n
    check = list(origins)
    for o in check:
        if visited[o]:
            raise ValueError("visited twice")
        visited[o] = True
    at = 0
    while at < len(check):  # lpKFtoCheck
        k = check[at]
        for c in children[k]:
            if visited[c]:
                raise ValueError("visited twice")
            visited[c] = True
            if not flag[c]:  # (:801)
                Tchildc = mul44(Tcw[c], Twc[k])  # (:803)
                T[c] = mul44(Tchildc, T[k])  # (:805)
                flag[c] = True
            check.append(c)
        at += 1
    # SetPose(mTcwGBA) reaches every key frame of the walk (:813), an origin outside the GBA included
    new = np.array([T[k] if flag[k] or visited[k] else np.asarray(Tcw[k], f32).reshape(4, 4) for k in range(n)], f32)
    return new, np.array(flag, np.uint8), np.array(visited, np.uint8)


def gba_update_points(xw, bad, in_gba, pos_gba, ref_kf, reached, Tcw_bef, Twc_new):
    """(:818-852) -> (xw_out, moved)"""
    out = np.asarray(xw, f32).copy()
    moved = np.zeros(len(out), np.uint8)
    for i in range(len(out)):
        if bad[i]:  # (:824)
            continue
        if in_gba[i]:  # (:827-831)
            out[i] = np.asarray(pos_gba[i], f32)
            moved[i] = 1
            continue
        r = ref_kf[i]
        if r < 0 or not reached[r]:  # (:837); r < 0: the reference would dereference NULL
            continue
        Xc = rigid_map(Tcw_bef[r], out[i])  # Rcw * P + tcw (:843)
        out[i] = rigid_map(Twc_new[r], Xc)  # Rwc * Xc + twc (:850)
        moved[i] = 2
    return out, moved
