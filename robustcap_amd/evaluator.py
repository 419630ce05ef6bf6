"""The motion evaluators of ``articulate/evaluator.py:155-394`` on the device: ``FullMotionEvaluator`` and the per-joint, mean-per-joint
and mesh evaluators, which are column views of the same quantities. One ``rc_motion_metrics`` call each (csrc/rc_motion.hip); the
per-joint, mean-per-joint and mesh evaluators also take the SVD alignments ``align_joint`` -1 .. -5 (evaluator.py:198-207, 301-310:
R/t/s, R/t, t/s, t, s), which are one ``rc_aligned_metrics`` call (csrc/rc_align.hip). This file converts the inputs with the
``body.*`` conversions and marshals pointers.

Not implemented (``NotImplementedError`` naming the argument): quaternion and Euler-angle inputs, ``use_pose_blendshape=True``, a
negative ``align_joint`` in ``FullMotionEvaluator`` (the reference declares it non-negative there), and different shapes for
prediction and truth (a context holds one body).
"""
import enum

import torch

from . import body as _body


class RotationRepresentation(enum.Enum):
    """articulate/math/angular.py:21-29"""
    AXIS_ANGLE = 0
    ROTATION_MATRIX = 1
    QUATERNION = 2
    R6D = 3
    EULER_ANGLE = 4


def _mask_bits(joint_mask):
    """the reference's ``joint_mask`` (a list / tensor of joint ids, or a boolean mask of 24 entries) as a bit mask; None -> 0"""
    if joint_mask is None:
        return 0
    m = torch.as_tensor(joint_mask).flatten()
    ids = m.nonzero().flatten().tolist() if m.dtype == torch.bool else [int(j) for j in m.tolist()]
    if any(j < 0 or j > 23 for j in ids) or len(set(ids)) != len(ids):
        raise ValueError("joint_mask: distinct joint ids in 0..23 (or a boolean mask of 24 entries) expected")
    return sum(1 << j for j in ids)


class _BasePoseEvaluator:
    def __init__(self, official_model_file=None, rep=RotationRepresentation.ROTATION_MATRIX, use_pose_blendshape=False, align_joint=0,
                 device="cuda", body=None, svd_align=False):
        if use_pose_blendshape:
            raise NotImplementedError("use_pose_blendshape=True: pose blendshapes are not implemented")
        rep = RotationRepresentation(rep.value if isinstance(rep, enum.Enum) else rep)
        if rep in (RotationRepresentation.QUATERNION, RotationRepresentation.EULER_ANGLE):
            raise NotImplementedError(f"rep={rep.name}: rotation matrices, axis angles and r6d are implemented")
        align_joint = align_joint if isinstance(align_joint, int) else align_joint.value
        if align_joint < 0 and not svd_align:
            raise NotImplementedError(f"align_joint={align_joint}: FullMotionEvaluator takes a joint id (the reference declares it non-negative)")
        if align_joint > 23:
            raise ValueError("align_joint must be a joint id in 0..23")
        self.model = _body.ParametricModel(official_model_file, device=device, body=body)
        self.rep, self.align_joint, self.device = rep, align_joint, torch.device(device)

    def _pose(self, pose):
        pose = torch.as_tensor(pose)
        n = pose.shape[0]
        if self.rep == RotationRepresentation.AXIS_ANGLE:
            return _body.axis_angle_to_rotation_matrix(pose.reshape(-1, 3), self.device).view(n, 24, 3, 3)
        if self.rep == RotationRepresentation.R6D:
            return _body.r6d_to_rotation_matrix(pose.reshape(-1, 6), self.device).view(n, 24, 3, 3)
        return pose.to(self.device, torch.float32).reshape(n, 24, 3, 3)

    def _shape(self, shape_p, shape_t):
        """one body for both motions: the shapes must be equal (None = the mean shape)"""
        if (shape_p is None) != (shape_t is None) or (shape_p is not None and not torch.equal(
                torch.as_tensor(shape_p, dtype=torch.float32).cpu().reshape(-1, 10), torch.as_tensor(shape_t, dtype=torch.float32).cpu().reshape(-1, 10))):
            raise NotImplementedError("shape_p / shape_t: different shapes for prediction and truth are not implemented")
        self.model.set_shape(shape_p)

    def _run(self, pose_p, pose_t, tran_p=None, tran_t=None, mesh=True, fps=60, joint_mask=0):
        return self.model.motion_metrics(self._pose(pose_p), self._pose(pose_t), tran_p, tran_t, fps=fps, align_joint=self.align_joint,
                                         joint_mask=joint_mask, mesh=mesh)

    def _run_aligned(self, pose_p, pose_t, mesh):
        """align_joint < 0 (evaluator.py:198-209, 301-312) on converted poses: (joint_err [1,24], mesh_err [1] or None); below -5 the
        reference's RuntimeError"""
        _body.align_bits(self.align_joint)
        return self.model.aligned_metrics(pose_p, pose_t, align=self.align_joint, mesh=mesh)


class PerJointErrorEvaluator(_BasePoseEvaluator):
    """articulate/evaluator.py:155-215: [3, 24] = position, local and global rotation error (degrees) of every joint. ``align_joint``
    -1 .. -5: the positions after the frame-wise R/t/s, R/t, t/s, t or s fit on the 24 joints; the two angle rows are those of
    ``align_joint=0``, bit for bit (the alignment does not touch them)."""

    def __init__(self, official_model_file=None, align_joint=0, rep=RotationRepresentation.ROTATION_MATRIX, device="cuda", body=None):
        super().__init__(official_model_file, rep, False, align_joint, device, body, svd_align=True)

    def __call__(self, pose_p, pose_t):
        if self.align_joint < 0:
            pose_p, pose_t = self._pose(pose_p), self._pose(pose_t)
            je, _ = self._run_aligned(pose_p, pose_t, mesh=False)
            _, pj = self.model.motion_metrics(pose_p, pose_t, align_joint=0, mesh=False)       # the angle rows: untouched by the alignment
            return torch.cat((je[:1], pj[0, 1:3])).cpu()
        _, pj = self._run(pose_p, pose_t, mesh=False)
        return pj[0, :3].cpu()


class MeanPerJointErrorEvaluator(PerJointErrorEvaluator):
    """articulate/evaluator.py:218-253: the mean over the joints of PerJointErrorEvaluator, [3]."""

    def __call__(self, pose_p, pose_t):
        return super().__call__(pose_p, pose_t).mean(dim=1)


class MeshErrorEvaluator(_BasePoseEvaluator):
    """articulate/evaluator.py:256-314: the mean vertex position error (align_joint position aligned; -1 .. -5: after the frame-wise
    R/t/s, R/t, t/s, t or s fit on all vertices)."""

    def __init__(self, official_model_file=None, align_joint=0, rep=RotationRepresentation.ROTATION_MATRIX, use_pose_blendshape=False,
                 device="cuda", body=None):
        super().__init__(official_model_file, rep, use_pose_blendshape, align_joint, device, body, svd_align=True)

    def __call__(self, pose_p, pose_t, shape_p=None, shape_t=None):
        self._shape(shape_p, shape_t)
        if self.align_joint < 0:
            return self._run_aligned(self._pose(pose_p), self._pose(pose_t), mesh=True)[1][0].cpu()
        out, _ = self._run(pose_p, pose_t)
        return out[0, 1, 0].cpu()


class FullMotionEvaluator(_BasePoseEvaluator):
    """articulate/evaluator.py:317-394: [11, 2] = (mean, mean over columns of the std over frames) of joint, vertex, local and global
    angle error, predicted and true jerk, one-second translation error, the three masked errors and the tracking error."""

    def __init__(self, official_model_file=None, align_joint=0, rep=RotationRepresentation.ROTATION_MATRIX, use_pose_blendshape=False,
                 fps=60, joint_mask=None, device="cuda", body=None):
        super().__init__(official_model_file, rep, use_pose_blendshape, align_joint, device, body)
        self.fps, self.joint_mask = int(fps), joint_mask
        self._mask = _mask_bits(joint_mask)

    def __call__(self, pose_p, pose_t, shape_p=None, shape_t=None, tran_p=None, tran_t=None):
        self._shape(shape_p, shape_t)
        out, _ = self._run(pose_p, pose_t, tran_p, tran_t, fps=self.fps, joint_mask=self._mask)
        return out[0].cpu()
