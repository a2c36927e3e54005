// vk_ws.h -- how a workspace is stated: its pieces one after another, each at a multiple of 256 bytes.  Plain C++, shared by
// vkimg.hip and the host-only plan headers (vk_bamplan.h).
#ifndef VK_WS_H
#define VK_WS_H

#include <cstddef>
#include <cstdint>

namespace {

size_t ws_align(size_t x) { return (x + 255) / 256 * 256; }
// Hands out the pieces of a workspace one after another, each at a multiple of 256 bytes.  A piece is stated once: the
// typed pointer it fills and its element count.  Without a base only the sizes add up (the *_workspace_size calls).
struct WsTake {
    uint8_t* base;
    size_t at;
    template <class T> void operator()(T*& piece, size_t count) {
        piece = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at += ws_align(count * sizeof(T));
    }
};

}  // namespace

#endif  // VK_WS_H
