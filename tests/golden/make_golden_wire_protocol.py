#!/usr/bin/env python3
"""The test platform's wire protocol as the REFERENCE'S OWN TEXT states it -> tests/golden/wire_protocol.json.

server.py cannot be imported (it needs cv2) and the firmware's C needs Xilinx headers, so the reference's sources are read AS TEXT
(nothing is imported, compiled or copied): every constant of the protocol is taken out of that text by a pattern that must match,
and only the values are stored.  tests/test_wire_protocol_pins.py checks the stand-in server and the board client against them.
Run where the reference is present:

    SGM_REFERENCE_DIR=<the reference's checkout> python tests/golden/make_golden_wire_protocol.py
"""
import json
import os
import re

REF = os.environ.get("SGM_REFERENCE_DIR", "")                 # the reference's checkout (as for oracle/build_ref.sh)
SERVER = os.path.join(REF, "HostScript_Server", "server.py")
FW_SRC = os.path.join(REF, "ZedBoard", "Vitis", "lwip_tcp_perf_client", "src")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wire_protocol.json")


def text(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def one(pattern, s, flags=0):
    m = re.search(pattern, s, flags)
    assert m, pattern
    return m


def main():
    assert os.path.isfile(SERVER), "set SGM_REFERENCE_DIR to the reference's checkout"
    ref = text(SERVER)
    fb = text(os.path.join(FW_SRC, "frame_buffer.h"))
    fw = text(os.path.join(FW_SRC, "tcp_perf_client.c"))
    sm = text(os.path.join(FW_SRC, "stereo_matching.c"))
    server = {}
    # image header server -> board (send_image)
    server["image_header_format"] = one(r"struct\.pack\('(<BiHH)',\s*type_id,\s*seq,\s*width,\s*height\)", ref).group(1)
    # close status (send_close_status)
    m = one(r"def send_close_status.*?struct\.pack\('(<B)',\s*(\d+)\)", ref, re.S)
    server["close_status_format"], server["close_status_value"] = m.group(1), int(m.group(2))
    # the calibration block follows the header only for this type
    server["calibration_after_type"] = int(one(r"if type_id == (\d+) and calib is not None:.*?conn\.send\(calib\.pack\(\)\)", ref, re.S).group(1))
    # planes: one loop over the channels and rows per image, left then right
    planes = re.findall(r"for ch in range\((\d+)\):\s*\n\s*for y in range\(height\):\s*\n\s*conn\.send\(img_(left|right)\[y, :, ch\]\.tobytes\(\)\)", ref)
    server["image_planes"] = [{"image": side, "channels": int(n), "order": "channel-major, then rows"} for n, side in planes]
    # result board -> server, after its type byte
    server["result_header_format"] = one(r"struct\.unpack\('(<iHH)',\s*header_bytes\)", ref).group(1)
    server["result_header_bytes"] = int(one(r"recv_exact\(conn, (\d+)\)", ref).group(1))
    server["result_row_bytes_per_pixel"] = int(one(r"row_size\s*=\s*width\s*\*\s*(\d+)", ref).group(1))
    server["result_row_dtype"] = one(r"np\.frombuffer\(row, dtype=np\.(\w+)\)", ref).group(1)
    # request codes the server answers
    server["request_codes"] = sorted({int(c) for c in re.findall(r"request == (\d+)", ref)})
    m = one(r"request == (\d+) or request == (\d+)", ref)
    server["image_request_codes"] = [int(m.group(1)), int(m.group(2))]
    server["width"] = int(one(r"^WIDTH = (\d+)$", ref, re.M).group(1))
    server["height"] = int(one(r"^HEIGHT = (\d+)$", ref, re.M).group(1))

    firmware = {}
    firmware["img_width"] = int(one(r"#define IMG_WIDTH (\d+)", fb).group(1))
    firmware["img_height"] = int(one(r"#define IMG_HEIGHT (\d+)", fb).group(1))
    # the receive state machine: header + calibration bytes, then the planes
    m = one(r"(\d+) \+ IMG_WIDTH \* IMG_HEIGHT \* (\d+)", fw)
    firmware["receive_prefix_bytes"], firmware["receive_planes"] = int(m.group(1)), int(m.group(2))
    # result header: type byte, then frame id, width, height: [header byte, right shift of the field] of every byte written
    firmware["result_type"] = int(one(r"header\[0\] = (\d+);", fw).group(1))
    firmware["result_field_bytes"] = {
        name: sorted([int(i), int(sh or 0)] for i, sh in
                     re.findall(rf"header\[(\d+)\] = \(uint8_t\)\(?shared_memory->last_depth_frame\.{name}(?: >> (\d+))?\)?;", fw))
        for name in ("frame_id", "width", "height")}
    firmware["result_bytes_per_pixel"] = int(one(r"IMG_HEIGHT \* IMG_WIDTH \* (\d+)", fw).group(1))
    # message types the firmware accepts from the server
    m = one(r"type == (\d+) \|\| type == (\d+)", fw)
    firmware["image_types"] = [int(m.group(1)), int(m.group(2))]
    firmware["other_types"] = sorted({int(c) for c in re.findall(r"type == (\d+)", fw)} - set(firmware["image_types"]))
    # grey conversion (stereo_matching.c): (wr R + wg G + wb B) >> shift as uint8, stored as float
    m = one(r"uint32_t gray =\s*(\d+)u\s*\*[^;]*?left_red\[i\]\s*\+\s*(\d+)u\s*\*[^;]*?left_green\[i\]\s*\+\s*(\d+)u\s*\*[^;]*?left_blue\[i\];", sm, re.S)
    firmware["grey_weights_rgb"] = [int(v) for v in m.groups()]
    firmware["grey_shift"] = int(one(r"uint8_t gray8 = \(uint8_t\)\(gray >> (\d+)\);", sm).group(1))
    one(r"depth\[i\] = \(float\)gray8;", sm)
    firmware["grey_stored_as"] = "float"

    doc = {"generator": "tests/golden/make_golden_wire_protocol.py",
           "source": "the reference's HostScript_Server/server.py and ZedBoard/Vitis/lwip_tcp_perf_client/src/{frame_buffer.h, "
                     "tcp_perf_client.c, stereo_matching.c}, read as text",
           "server": server, "firmware": firmware}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
