"""Joint names and feature masks of the HumanML3D vector (the data the reference's data_loaders/humanml_utils.py holds), written from the layout of
the 263 rows (data_loaders/humanml/scripts/motion_process.py:355-361; csrc/rgn_hml_check.h):

    row 0                      rotation velocity of the root
    rows 1, 2                  root velocity (x, z)
    row 3                      root height
    3 (J-1) rows               local positions of joints 1 .. J-1, (x, y, z) each
    6 (J-1) rows               rotations of joints 1 .. J-1, six numbers each
    3 J rows                   velocities of joints 0 .. J-1, (x, y, z) each
    4 rows                     foot contacts

A mask holds True for the rows that belong to a set of joints. HML_ROOT_MASK: the four root rows and the root's velocity. HML_LOWER_BODY_MASK: the
root rows, every block's rows of the lower-body joints, and the foot contacts; sample/edit.py's upper_body mode keeps exactly those rows of the
input (True = keep) and generates the rest. tests/test_hml_cpu.py compares all three with the reference's arrays."""
import numpy as np

HML_JOINT_NAMES = [
    "pelvis", "left_hip", "right_hip", "spine1", "left_knee", "right_knee", "spine2", "left_ankle", "right_ankle", "spine3", "left_foot",
    "right_foot", "neck", "left_collar", "right_collar", "head", "left_shoulder", "right_shoulder", "left_elbow", "right_elbow", "left_wrist",
    "right_wrist",
]
NUM_HML_JOINTS = len(HML_JOINT_NAMES)           # the 22 SMPL-H body joints
HML_LOWER_BODY_NAMES = ("pelvis", "left_hip", "right_hip", "left_knee", "right_knee", "left_ankle", "right_ankle", "left_foot", "right_foot")
HML_LOWER_BODY_JOINTS = [HML_JOINT_NAMES.index(n) for n in HML_LOWER_BODY_NAMES]
SMPL_UPPER_BODY_JOINTS = [j for j in range(NUM_HML_JOINTS) if j not in HML_LOWER_BODY_JOINTS]


def feature_mask(joints, root_rows, contacts, num_joints=NUM_HML_JOINTS):
    """bool [12 J - 1]: the rows of `joints` in the position, rotation and velocity blocks, the four root rows when root_rows, the four contact
    rows when contacts."""
    member = np.zeros(num_joints, dtype=bool)
    member[list(joints)] = True
    return np.concatenate((np.full(4, bool(root_rows)), np.repeat(member[1:], 3), np.repeat(member[1:], 6), np.repeat(member, 3),
                           np.full(4, bool(contacts))))


HML_ROOT_MASK = feature_mask([0], root_rows=True, contacts=False)
HML_LOWER_BODY_MASK = feature_mask(HML_LOWER_BODY_JOINTS, root_rows=True, contacts=True)
HML_UPPER_BODY_MASK = ~HML_LOWER_BODY_MASK
