"""The test platform's wire protocol, pinned against the REFERENCE'S OWN TEXT.

server.py cannot be imported here (it needs cv2), and the firmware's C needs Xilinx headers -- so the board client
(csrc/sgm_board_client.c) is exercised against a stand-in server (tests/platform_server.py).  What keeps the stand-in and the client
honest is this file: every constant of the protocol -- struct formats, type codes, image size, the calibration block's place and size,
the byte order of the result header -- as tests/golden/make_golden_wire_protocol.py read it out of the reference's sources (as text:
nothing imported, compiled or copied) into tests/golden/wire_protocol.json, checked against what the stand-in sends and the client
parses."""
import json
import os
import struct

from conftest import GOLDEN, ROOT


def text(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def pinned():
    with open(os.path.join(GOLDEN, "wire_protocol.json")) as f:
        return json.load(f)


def test_server_side_formats_match_the_stand_in_and_the_client():
    ref = pinned()["server"]
    ours = text(os.path.join(ROOT, "tests", "platform_server.py"))
    client = text(os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc", "sgm_board_client.c"))
    # image header server -> board: type (1 B), seq (int32), width, height (uint16), little-endian (server.py send_image)
    assert ref["image_header_format"] == "<BiHH"
    assert 'struct.pack("<BiHH", type_id, seq, w, h)' in ours and struct.calcsize("<BiHH") == 9
    assert "uint8_t hdr[9];" in client and "hdr[5] | (hdr[6] << 8)" in client and "hdr[7] | (hdr[8] << 8)" in client
    # close status: one zero byte (send_close_status); the client stops on type 0
    assert ref["close_status_format"] == "<B" and ref["close_status_value"] == 0
    assert 'struct.pack("<B", 0)' in ours and "if (hdr[0] == 0) break;" in client
    # the calibration block follows the header only for type 1 (server.py: `if type_id == 1 and calib is not None: conn.send(calib.pack())`)
    assert ref["calibration_after_type"] == 1
    assert "if (hdr[0] == 1) {" in client and "recv_all(fd, cal, 80)" in client
    # planes: left B, G, R then right B, G, R, each `height` rows of `width` bytes (two loops over range(3) x range(height))
    assert [(p["image"], p["channels"]) for p in ref["image_planes"]] == [("left", 3), ("right", 3)]
    # result board -> server: type byte 3 already read, then <iHH (seq, width, height), then height rows of width float32
    assert ref["result_header_format"] == "<iHH" and ref["result_header_bytes"] == 8 == struct.calcsize("<iHH")
    assert ref["result_row_bytes_per_pixel"] == 4 and ref["result_row_dtype"] == "float32"
    assert 'struct.unpack("<iHH", self._recv(conn, 8))' in ours
    assert "uint8_t out[9] = {3, hdr[1], hdr[2], hdr[3], hdr[4], hdr[5], hdr[6], hdr[7], hdr[8]};" in client
    # request codes the server answers: 1 = image + calibration, 2 = image, 3 = result follows, 0 = stop
    assert {0, 1} <= set(ref["request_codes"]) and ref["image_request_codes"] == [1, 2]
    # the platform's fixed frame size
    assert ref["width"] == 1280 and ref["height"] == 720


def test_firmware_side_constants_match_the_client():
    fw = pinned()["firmware"]
    client = text(os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc", "sgm_board_client.c"))
    assert fw["img_width"] == 1280 and fw["img_height"] == 720
    # the firmware's receive state machine: 9 header bytes + 80 calibration bytes = 89, then six planes
    assert fw["receive_prefix_bytes"] == 89 and fw["receive_planes"] == 6
    assert struct.calcsize("<BiHH") + 20 * 4 == 89
    # its result header: byte 0 = 3, frame id little-endian in bytes 1..4, width in 5..6, height in 7..8; then W*H*4 bytes of depth
    assert fw["result_type"] == 3 and fw["result_field_bytes"] == {"frame_id": [[1, 0], [2, 8], [3, 16], [4, 24]],
                                                                   "width": [[5, 0], [6, 8]], "height": [[7, 0], [8, 8]]}
    assert fw["result_bytes_per_pixel"] == 4
    assert "uint8_t out[9] = {3," in client
    # message types the firmware accepts from the server
    assert fw["image_types"] == [1, 2] and {0, 3} <= set(fw["other_types"])


def test_firmware_grey_conversion_weights():
    """stereo_matching.c:15-24 (the file needs Xilinx headers, so it is read, not built): grey = (76 R + 150 G + 29 B) >> 8 as uint8,
    stored as float -- the weights of sgm_gray_planes_k's board mode, of oracle/platform_oracle.board_gray and of --placeholder-gray."""
    import numpy as np
    from oracle.platform_oracle import board_gray
    fw = pinned()["firmware"]
    assert tuple(fw["grey_weights_rgb"]) == (76, 150, 29)
    assert fw["grey_shift"] == 8 and fw["grey_stored_as"] == "float"
    r, g, b = np.array([255, 0, 13], np.uint8), np.array([255, 0, 200], np.uint8), np.array([255, 0, 77], np.uint8)
    assert board_gray(b, g, r, 76).tolist() == [(76 * 255 + 150 * 255 + 29 * 255) >> 8, 0, (76 * 13 + 150 * 200 + 29 * 77) >> 8]
    client = text(os.path.join(ROOT, "soc_project_stereo_matching_amd", "csrc", "sgm_board_client.c"))
    assert "76" in client and "150" in client and "29" in client
