// empty on purpose: tests/emul/adapter_emul.cpp compiles csrc/vk_adapter.h for the host and states itself what that
// header takes from HIP
